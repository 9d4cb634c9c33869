"""numpy RESTATEMENT of the keyed Dropout, written from the text of include/hsp.h (hsp_dropout_keyed_fwd in the section "keyed
draws of a step"), not from the kernel; fmix32 / absorb / the instance key / the fp32 uniform are tests/_step_draws_ref.py's."""
import numpy as np

from _sample_ids_ref import instance_key
from _step_draws_ref import uniform_f32, words

DROP_J, DROP_TAG = 0x83000000, 0xfffffffa
SITES = dict(Rot_green=0, Rot_red=1, Pose_Ts=2)


def scale_of(p):
    """1 / (1 - p), computed once in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed, call, site, p, R, C):
    """-> (R,C) bool: element i = r C + c keeps iff the fp32 uniform of word(i) >= p"""
    u = uniform_f32(words(instance_key(seed, call, DROP_J | site), DROP_TAG, np.arange(R * C, dtype=np.uint32)))
    return (u >= np.float32(p)).reshape(R, C)


def dropout(x, seed, call, site, p):
    """x (R,C) fp32 -> (out (R,C) fp32, keep (R,C) uint8)"""
    x = np.asarray(x, dtype=np.float32)
    keep = keep_mask(seed, call, site, p, *x.shape)
    out = np.where(keep, (x * scale_of(p)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return out, keep.astype(np.uint8)
