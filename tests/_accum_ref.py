"""Gradient accumulation of the graphed training step, stated in plain Python: which slots are skipped, taken and applied
(include/hsp.h, hsp_step_gate_accum, rules 1-7; engine/train.py:99-114 of the reference, quirks included) and what the take does
to the accumulator (hsp_grad_accumulate's formula in numpy fp32).  No device, no library: tests/test_accumulate_host.py holds
``decisions`` to a literal run of the reference's loop, the GPU tests hold the kernels to this file.

An EVENT is what one replay found: 'ok', 'nan' (the total loss is NaN) or 'noitem' (no item of the batch was good).
"""
import numpy as np

OK, NAN, NOITEM = "ok", "nan", "noitem"


def decisions(accumulate, global_step0, events, horizon):
    """One dict per slot, the state AFTER that replay of an armed gate: take / first / apply / index and the running micro,
    pending, applied, replays, skipped_nan, skipped_no_item, exhausted.

      * ``micro`` plays the reference's ``global_step``: it starts at ``global_step0`` and advances on every slot.
      * skipped slot (NaN loss, no good item): nothing enters the accumulator, nothing is applied.
      * table used up (``applied >= horizon``): exhausted = 1, nothing taken, nothing applied.
      * taken slot: first = nothing was pending; the step is applied exactly when ``micro % accumulate == 0`` (slot 0 steps on
        its own gradient alone), and then nothing is pending any more; a skipped stepping slot leaves the accumulator growing
        until the next ``micro % accumulate == 0``."""
    if accumulate < 1 or horizon < 1:
        raise ValueError("decisions: expects accumulate >= 1 and horizon >= 1")
    micro, pending, applied, index = int(global_step0), 0, 0, 0
    replays = skipped_nan = skipped_no_item = exhausted = 0
    out = []
    for ev in events:
        replays += 1
        take = first = apply = 0
        if ev == NAN:
            skipped_nan += 1
        elif ev == NOITEM:
            skipped_no_item += 1
        elif ev != OK:
            raise ValueError(f"decisions: unknown event {ev!r}")
        elif applied >= horizon:
            exhausted = 1
        else:
            take, first = 1, int(pending == 0)
            pending += 1
            if micro % accumulate == 0:
                apply, index = 1, applied
                applied += 1
                pending = 0
        micro += 1
        out.append(dict(take=take, first=first, apply=apply, index=index, micro=micro, pending=pending, applied=applied,
                        replays=replays, skipped_nan=skipped_nan, skipped_no_item=skipped_no_item, exhausted=exhausted))
    return out


def _events(n, nan=(), noitem=()):
    return [NAN if i in nan else NOITEM if i in noitem else OK for i in range(n)]


# (name, global_step0, events, horizon): shared by the host test and the GPU gate test, run at accumulate 1, 2, 3 and 4
EVENT_CASES = (
    ("nan-on-slot-0", 0, _events(13, nan=(0,)), 100),                 # micro 0: a stepping slot at every accumulate
    ("nan-on-slot-12", 0, _events(14, nan=(12,)), 100),               # micro 12: stepping at 2, 3 and 4, after full rounds
    ("nan-on-slot-1", 0, _events(13, nan=(1,)), 100),                 # micro 1: accumulate-only at 2, 3 and 4
    ("two-nans-in-a-row", 0, _events(13, nan=(4, 5)), 100),
    ("nans-over-a-whole-round", 0, _events(14, nan=(3, 4, 5, 6)), 100),
    ("offset-start", 5, _events(12, nan=(3,)), 100),                  # global_step0 = 5: a multiple of none of 2, 3, 4
    ("no-item", 0, _events(12, noitem=(2, 6), nan=(7,)), 100),
    ("exhaustion", 0, _events(14, nan=(9,)), 2),
    ("exhaustion-offset", 3, _events(12), 1),
)


def clip_coef(norm_sq, max_norm):
    """min(1, max_norm / (sqrt(norm_sq) + 1e-6)) in fp32, one rounding per operation; a NaN norm gives a NaN coefficient"""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.sqrt(np.float32(norm_sq)) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def accumulate(acc, fresh, first, prev_norm_sq, max_norm):
    """hsp_grad_accumulate's element formula: first ? 0 + fresh : fl(fl(acc * c) + fresh), numpy fp32 (no fused multiply-add)"""
    acc, fresh = np.asarray(acc, dtype=np.float32), np.asarray(fresh, dtype=np.float32)
    with np.errstate(all="ignore"):
        if first:
            return np.float32(0.0) + fresh
        scaled = (acc * clip_coef(prev_norm_sq, max_norm)).astype(np.float32)
        return (scaled + fresh).astype(np.float32)
