"""CPU: the renderer's entry points (include/hsp.h: hsp_render_depth_*, hsp_label_boxes) refuse bad arguments with their error
codes before any launch -- nothing here needs a GPU --, and the workspace query answers the sizes the header names."""
import ctypes

import pytest

null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)


def render_args(**kw):
    """a call every check passes (on made-up addresses: it is never sent) with the named arguments replaced"""
    a = dict(verts=one, V=8, tris=one, T=12, mesh=one, n_mesh=1, mesh_id=one, frame_id=one, label=one, rt=one, scale=one, camK=one,
             camK_rows=1, n=2, F=3, H=48, W=64, over=0, depth=one, labels=one, ws=one, ws_bytes=1 << 30, stream=null)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("entry", ["hsp_render_depth_u16", "hsp_render_depth_f32"])
def test_render_refuses_bad_arguments(entry):
    from hs_pose_amd._lib import ERR_BAD_ARG, ERR_WORKSPACE, lib
    fn = getattr(lib(), entry)
    for name in ("verts", "tris", "mesh", "mesh_id", "frame_id", "label", "rt", "scale", "camK", "depth", "labels"):
        assert fn(*render_args(**{name: null})) == ERR_BAD_ARG, name
    for kw in (dict(n=-1), dict(n=65536), dict(F=0), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(over=2), dict(over=-1),
               dict(camK_rows=2), dict(camK_rows=0), dict(V=0), dict(T=0), dict(n_mesh=0)):
        assert fn(*render_args(**kw)) == ERR_BAD_ARG, kw
    for kw in (dict(ws=null), dict(ws_bytes=1000), dict(ws=ctypes.c_void_p(72))):
        assert fn(*render_args(**kw)) == ERR_WORKSPACE, kw
    # n == 0 reads no instance: its pointers may be NULL, but the frames and the workspace are still checked
    none = dict(verts=null, tris=null, mesh=null, mesh_id=null, frame_id=null, label=null, rt=null, scale=null, camK=null, n=0)
    assert fn(*render_args(depth=null, **none)) == ERR_BAD_ARG
    assert fn(*render_args(ws_bytes=0, **none)) == ERR_WORKSPACE


def test_label_boxes_refuses_bad_arguments():
    from hs_pose_amd._lib import ERR_BAD_ARG, lib
    fn = lib().hsp_label_boxes
    good = [one, one, one, 2, 3, 48, 64, one, one, null]
    for i in (0, 1, 2, 7, 8):
        assert fn(*(good[:i] + [null] + good[i + 1:])) == ERR_BAD_ARG, i
    for i, v in ((3, 0), (3, 65536), (4, 0), (5, 0), (6, 0)):
        assert fn(*(good[:i] + [v] + good[i + 1:])) == ERR_BAD_ARG, (i, v)
    assert fn(one, one, one, 2, 3, 65536, 32768, one, one, null) == ERR_BAD_ARG          # H * W >= 2^31


def test_workspace_query():
    from hs_pose_amd._lib import lib
    q = lib().hsp_render_workspace_bytes
    assert q(0, 48, 64, 1) == 0 and q(1, 0, 64, 1) == 0 and q(1, 48, 64, -1) == 0 and q(1, 48, 64, 65536) == 0
    assert q(1, 65536, 32768, 1) == 0
    a, b = q(1, 48, 64, 0), q(3, 48, 64, 5)
    assert a >= 48 * 64 * 8 and b >= 3 * 48 * 64 * 8 + 6 * 8 and b > a and a % 16 == 0 and b % 16 == 0
    assert q(24, 480, 640, 48) >= 24 * 480 * 640 * 8


def test_ops_refuse_cpu_tensors():
    import torch
    from hs_pose_amd import ops, render
    from hs_pose_amd._lib import HspError
    z = torch.zeros
    with pytest.raises(HspError, match="GPU tensor"):
        ops.render_depth(z(8, 3), z(12, 3, dtype=torch.int32), z(1, 4, dtype=torch.int32), z(1, dtype=torch.int32),
                         z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(1, 4, 4), z(1, 3), z(1, 9, dtype=torch.float64), 1, 48, 64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.label_boxes(z(1, 48, 64, dtype=torch.uint8), z(1, dtype=torch.int32), z(1, dtype=torch.int32))
    ms = render.MeshSet([render.shapes.box()], device="cpu")
    with pytest.raises(HspError, match="GPU tensor"):
        render.render_frames(ms, [0], torch.eye(4)[None], torch.ones(1, 3), torch.eye(3, dtype=torch.float64), 48, 64)
