"""GPU: the row-copy, column-sum and reverse-index kernels of csrc/gather.hip (outside its scatter-tile / ORL / points-max part)
and csrc/csr.hip against the references of tests/_rows_ref.py, which are written from the formulas of include/hsp.h in numpy /
torch fp64 and call no kernel (tests/test_rows_reference_host.py holds them to independent torch compositions).  Calls go through
the C ABI.

    column sums     hsp_colsum_rows, _bf16, _xyz, _xyz_bf16, hsp_colsum_cloud_f32 (with and without xyz): fp64 sums of the stored
                    values, per element within D u T / (1 - D u), u = 2^-24, T = sum|t_i|, D = ceil(rows / row_lanes) +
                    (row_lanes - 1) + ceil(nchunk / 8) + 3 from hsp_colsum_rows_plan (a moment slot: D + 1) -- derived, not
                    measured.  Every column's largest term sits on an EDGE row (a chunk's last row, the cloud's last row, the
                    last chunk's first row) and is at least four bounds large (checked on the host for every case), so a kernel
                    that drops or doubles one edge row fails.  The one-launch form equals the two-launch result bit for bit.
    row assembly    hsp_concat_rows, _pitched, _bf16: bit for bit a plain indexed copy, in the form (16-byte chunks, element
                    pairs, scalars) the documented conditions give for the call; the 16-byte form zeroes every padding column,
                    the others leave the padding alone.
    row gather      hsp_gather_rows_fwd: bit for bit.  hsp_gather_rows_bwd on its memset + atomic fallback: fp64 index_add within
                    n_m 2^-24 sum|g| (n_m the row's list length: any order of the adds), unselected rows exactly zero.
                    hsp_gather_rows_bwd_csr, _bf16, _multi, _multi_bf16: bit for bit a serial fp32 sum in ascending query order
                    (bf16: rounded once) over the numpy reverse map.
    reverse map     hsp_rev_build, _sel, _multi: the whole of rev_off and rev_edge equal to cumsum(bincount) / stable argsort,
                    edges in LDS and in global memory (hsp_rev_build_edges_in_lds asserts which).
    fused passes    hsp_residual_bias: bit for bit out + (f + t[b]); hsp_add_relu_bwd: bit for bit (ga + gb) * [y > 0].

Every output is a NaN-prefilled (int32: -1) view inside a parent of sentinels: the sentinels are intact after every call and a
declined call leaves the view as it was.  No case feeds an index out of range.

Measured err / (2^-24 sum|t|), worst over the cases of this file on an MI355X (recorded, not asserted; the bound allows D):
    hsp_colsum_rows       four-column form 2.0    scalar form 2.4         hsp_colsum_rows_bf16  0.34
    hsp_colsum_rows_xyz   sums 2.0   moments 2.5                          hsp_colsum_rows_xyz_bf16   sums 0.34   moments 2.4
    hsp_colsum_cloud_f32  sums 2.4   with xyz: sums 2.4   moments 3.1     (D of the cases: 5 ... 422)
    hsp_gather_rows_bwd, memset + atomics: 3.7 against its bound of n_m (up to 300)
    The worst ratios are clouds of a few rows (3 ... 8 terms); at thousands of rows they are 0.1 ... 0.8.  bf16 rows are exact in
    fp32 until the sum outgrows 24 bits, hence the small ratio.
The same table is in DESIGN.md section 2.0a.
"""
import ctypes

import numpy as np
import pytest
import torch

import _rows_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
I32 = torch.int32
NAN = float("nan")
SENTINEL = -1.2345678e30
ISENT = 0x5A5A5A5A
LEAD = 32
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
RATIOS = {}                                  # form -> worst measured err / (2^-24 sum|t|), printed by the last test


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _vp(t):
    """the address of a NAMED tensor: a temporary would be freed, and its block handed to the next allocation, before the launch"""
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() if torch.is_tensor(t) else t for t in ts]), ctypes.c_void_p)


def _ints(vs):
    return ctypes.cast((ctypes.c_int * len(vs))(*[int(v) for v in vs]), ctypes.c_void_p)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


def _same_bits(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {a.numel()} elements differ, first at {i}: got {got.cpu()[i].item()!r}, "
                             f"want {want.cpu()[i].item()!r}")


# ---- moats ------------------------------------------------------------------------------------------------------------------------

class Out:
    """a prefilled (rows, cols) output with row pitch ld inside a parent of sentinels; lead: elements before the view (the parent
    starts on 256 bytes, so LEAD + 1 is a base off by one element).  Float views are prefilled with NaN, int32 views with -1."""

    def __init__(self, rows, cols, ld, dev, dtype=F32, lead=LEAD, init=None):
        self.floating = dtype.is_floating_point
        self.lead = lead
        self.parent = torch.full((lead + rows * ld + LEAD,), SENTINEL if self.floating else ISENT, dtype=dtype, device=dev)
        assert self.parent.data_ptr() % 256 == 0
        self.v = self.parent.as_strided((rows, cols), (ld, 1), lead)
        if init is None:
            self.v.fill_(NAN if self.floating else -1)
        else:
            self.v.copy_(init)
        self.start = self.v.clone()
        self.before = self._outside()

    def _outside(self):
        p = self.parent.clone()
        p.as_strided(self.v.shape, self.v.stride(), self.lead).zero_()
        return _bits(p)

    def intact(self):
        return torch.equal(self._outside(), self.before)

    def untouched(self):
        return self.intact() and torch.equal(_bits(self.v), _bits(self.start))


class Ws:
    """a workspace of exactly `nbytes` bytes with a sentinel band behind it"""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)

    def intact(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _at(t, dev, off=0, ld=None):
    """t on the device: dense at `off` elements past a 256-byte boundary, or (2-d, ld given) as rows of pitch ld; the parent is
    NaN (floats) / the int sentinel elsewhere and stays alive with the view"""
    t = t.contiguous()
    fill = NAN if t.dtype.is_floating_point else ISENT
    if ld is None:
        parent = torch.full((off + t.numel() + LEAD,), fill, dtype=t.dtype, device=dev)
        v = parent[off:off + t.numel()].view(t.shape)
    else:
        rows, cols = t.shape
        parent = torch.full((off + rows * ld + LEAD,), fill, dtype=t.dtype, device=dev)
        v = parent.as_strided((rows, cols), (ld, 1), off)
    assert parent.data_ptr() % 256 == 0
    v.copy_(t)
    return v


# ======================================================================================================================================
# 1 / 2  column sums
# ======================================================================================================================================

def plan(B, N, C, eb):
    v = [ctypes.c_int(-7) for _ in range(4)]
    assert _L().hsp_colsum_rows_plan(B, N, C, eb, *[ctypes.byref(x) for x in v]) == OK
    return tuple(x.value for x in v)


def _colsum_call(form, x, xyz, dev, ws_scale=1):
    """the two-launch entry point of `form` ("rows", "rows_bf16", "xyz", "xyz_bf16") or the one-launch form ("cloud"); x, xyz on
    the CPU as stored -> (rc, Out)"""
    B, N, C = x.shape
    slots = 4 if xyz is not None else 1
    out = Out(B, slots * C, slots * C, dev)
    xd, wd = x.to(dev), (xyz.to(dev) if xyz is not None else None)
    L = _L()
    if form == "cloud":
        rc = L.hsp_colsum_cloud_f32(_vp(xd), _vp(wd), B, N, C, _vp(out.v), _stream())
    else:
        ws = Ws(slots * L.hsp_orl_workspace_bytes(B, N, C), dev)
        fn = {"rows": L.hsp_colsum_rows, "rows_bf16": L.hsp_colsum_rows_bf16, "xyz": L.hsp_colsum_rows_xyz,
              "xyz_bf16": L.hsp_colsum_rows_xyz_bf16}[form]
        args = (_vp(xd), _vp(wd)) if xyz is not None else (_vp(xd),)
        rc = fn(*args, B, N, C, _vp(out.v), _vp(ws.buf), ws.nbytes, _stream())
        torch.cuda.synchronize()
        assert ws.intact(), f"{form}: wrote behind its workspace"
    torch.cuda.synchronize()
    assert out.intact(), f"{form} {tuple(x.shape)}: wrote outside its output"
    return rc, out


def _hold_colsum(got, x, xyz, rows, lanes, nchunk, what, key, skip=None):
    """|got - want| <= D u T / (1 - D u) element by element; skip: a (B, C) mask of columns not held (non-finite inputs)"""
    B, N, C = x.shape
    mom = xyz is not None
    want, T = R.colsum_ref(x, xyz)
    tol = R.colsum_tol(T, R.colsum_depth(rows, lanes, nchunk), mom)
    got = got.detach().cpu().double().view(want.shape)
    keep = torch.ones_like(want, dtype=torch.bool)
    if skip is not None:
        keep &= ~(skip[:, None, :] if mom else skip)
    assert torch.isfinite(got[keep]).all(), f"{what}: non-finite (a sentinel left behind?)"
    err = torch.where(keep, (got - want).abs(), torch.zeros_like(want))
    pos = keep & (T > 0)
    ratio = (err[pos] / (R.U * T[pos])).max().item() if pos.any() else 0.0
    for k in ([key] if not mom else [key + " sums", key + " moments"]):
        r = ratio
        if mom:
            sl = slice(0, 1) if k.endswith("sums") else slice(1, 4)
            p = pos[:, sl]
            r = (err[:, sl][p] / (R.U * T[:, sl][p])).max().item() if p.any() else 0.0
        RATIOS[k] = max(RATIOS.get(k, 0.0), r)
    print(f"  {what}: rows {rows} lanes {lanes} nchunk {nchunk}  err / (u T) {ratio:.3f}  (D = {R.colsum_depth(rows, lanes, nchunk)})")
    over = torch.where(keep, err - tol, torch.full_like(err, -1.0))
    i = over.argmax()
    assert over.flatten()[i] <= 0, (f"{what}: |err| {err.flatten()[i]:.3e} > bound {tol.flatten()[i]:.3e} at "
                                    f"{np.unravel_index(int(i), over.shape)} (want {want.flatten()[i]:.6e})")


def _form_widths():
    return [(f, C) for f in R.FORMS for C in R.VEC_WIDTHS + (R.SCALAR_WIDTHS if f == "rows" else ())]


@pytest.mark.parametrize("form,C", _form_widths(), ids=lambda v: str(v))
def test_colsum_two_launch_forms(dev, form, C):
    dtype = BF if form.endswith("bf16") else F32
    eb = 2 if dtype == BF else 4
    with_xyz = form.startswith("xyz")
    want_form = 0 if C in R.VEC_WIDTHS else 1
    for B, N, kind, seed in R.colsum_cases(plan, form, C):
        rows, nchunk, lanes, f = plan(B, N, C, eb)
        assert f == want_form and (not with_xyz or _L().hsp_colsum_rows_xyz_takes(C))       # the route this case enters
        x, xyz = R.colsum_data(B, N, C, kind, seed, rows, nchunk, dtype, with_xyz)
        rc, out = _colsum_call(form, x, xyz, dev)
        assert rc == OK, (form, B, N, C, rc)
        key = form + (" scalar" if want_form else "")
        _hold_colsum(out.v, x, xyz, rows, lanes, nchunk, f"{form} ({B},{N},{C}) {kind}", key)


@pytest.mark.parametrize("form,C", [("rows", 260), ("rows", 2048), ("rows_bf16", 48), ("xyz", 48), ("xyz_bf16", 48), ("rows_bf16", 6),
                                    ("cloud", 16), ("cloud", 48), ("cloud_xyz", 16), ("cloud_xyz", 48)])
def test_colsum_declines_write_nothing(dev, form, C):
    B, N = 3, 40
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, N, C, generator=g).to(BF if form.endswith("bf16") else F32)
    xyz = torch.randn(B, N, 3, generator=g) if "xyz" in form else None
    if form.startswith("cloud"):
        assert _L().hsp_colsum_cloud_ok(B, N, C, int(xyz is not None)) == 0
    elif form.startswith("rows"):
        assert plan(B, N, C, x.element_size())[3] == -1
    else:
        assert _L().hsp_colsum_rows_xyz_takes(C) == 0
    rc, out = _colsum_call("cloud" if form.startswith("cloud") else form, x, xyz, dev)
    assert rc == UNSUPPORTED and out.untouched()


@pytest.mark.parametrize("with_xyz", [0, 1], ids=["sums", "xyz"])
@pytest.mark.parametrize("C", R.CLOUD_WIDTHS)
def test_colsum_cloud_form(dev, C, with_xyz):
    """the one-launch form: the fp64 bound, the two-launch result bit for bit, the largest cloud it accepts and the first it
    refuses (found by asking hsp_colsum_cloud_ok)"""
    ok = _L().hsp_colsum_cloud_ok
    for B, N, kind, seed, quiet, accepted in R.cloud_cases(plan, ok, C, with_xyz):
        assert ok(B, N, C, with_xyz) == int(accepted)
        rows, nchunk, lanes, f = plan(B, N, C, 4)
        assert f == 0
        x, xyz = R.colsum_data(B, N, C, kind, seed, rows, nchunk, F32, bool(with_xyz), quiet)
        rc, out = _colsum_call("cloud", x, xyz, dev)
        if not accepted:
            assert rc == UNSUPPORTED and out.untouched(), (B, N, C)
            continue
        assert rc == OK, (B, N, C, rc)
        _hold_colsum(out.v, x, xyz, rows, lanes, nchunk, f"cloud{' xyz' if with_xyz else ''} ({B},{N},{C}) {kind}",
                     "cloud_xyz" if with_xyz else "cloud")
        rc2, two = _colsum_call("xyz" if with_xyz else "rows", x, xyz, dev)
        assert rc2 == OK
        _same_bits(out.v, two.v, f"one launch against two ({B},{N},{C})")


@pytest.mark.parametrize("form", ["rows", "xyz", "cloud", "cloud_xyz", "rows_bf16"])
def test_colsum_non_finite_stays_in_its_column(dev, form):
    B, N, C = 3, 300, 64
    dtype = BF if form.endswith("bf16") else F32
    with_xyz = "xyz" in form
    rows, nchunk, lanes, _ = plan(B, N, C, 2 if dtype == BF else 4)
    x, xyz = R.colsum_data(B, N, C, "range", 77, rows, nchunk, dtype, with_xyz)
    x[1, 17, 5] = float("inf")
    x[1, 200, 9] = NAN
    rc, out = _colsum_call("cloud" if form.startswith("cloud") else form, x, xyz, dev)
    assert rc == OK
    got = out.v.cpu().view(B, -1, C)
    assert got[1, 0, 5].item() == float("inf") and torch.isnan(got[1, 0, 9])
    assert not torch.isfinite(got[1, :, 5]).any() and not torch.isfinite(got[1, :, 9]).any()
    skip = torch.zeros(B, C, dtype=torch.bool)
    skip[1, 5] = skip[1, 9] = True
    clean = x.clone()
    clean[1, 17, 5] = clean[1, 200, 9] = 0
    _hold_colsum(out.v, clean, xyz, rows, lanes, nchunk, f"{form} with inf / NaN", form + " (non-finite case)", skip=skip)
    assert torch.isfinite(got[~skip[:, None, :].expand_as(got)]).all()


# ======================================================================================================================================
# 3  row assembly
# ======================================================================================================================================

def _seg(kind, width, B, N, g, dtype=F32, nsrc=None, off=0, ids=None):
    """one column segment with random content; off: the source base off a 16-byte boundary by so many elements"""
    if kind == 0:
        return dict(kind=0, width=width, src=torch.randn(B * N, width, generator=g).to(dtype), off=off)
    if kind == 1:
        idx = torch.randint(0, nsrc, (B, N), generator=g, dtype=I32)
        idx[:, 0] = nsrc - 1                                             # rows 0 and nsrc - 1, and repeats wherever N > nsrc
        idx[:, -1] = 0
        if N > 2:
            idx[:, N // 2] = idx[:, 0]
        return dict(kind=1, width=width, src=torch.randn(B * nsrc, width, generator=g).to(dtype), idx=idx.reshape(-1), nsrc=nsrc, off=off)
    if kind == 2:
        return dict(kind=2, width=width, src=torch.randn(B, width, generator=g), off=off)
    ids = torch.randint(0, width, (B,), generator=g).float() if ids is None else torch.tensor(ids, dtype=F32)
    return dict(kind=3, width=width, src=ids, off=off)


def _run_concat(segs, B, N, pad, dev, dtype=F32, out_lead=LEAD, plain=False, expect=None):
    """run one assembly and hold it: the expected form from the documented conditions, the copy bit for bit, the padding by the
    form, the moats.  Returns the form."""
    eb = 2 if dtype == BF else 4
    used = sum(s["width"] for s in segs)
    pitch = used + pad
    srcs = [_at(s["src"], dev, s["off"]) for s in segs]
    idxs = [s["idx"].to(dev) if s["kind"] == 1 else None for s in segs]
    out_addr = out_lead * eb                                             # modulo 256: the parent starts on 256 bytes
    form = R.concat_form(eb, pitch, [(s["kind"], s["width"], t.data_ptr()) for s, t in zip(segs, srcs)], out_addr)
    if expect is not None:
        assert form == expect, (form, expect)
    cols = pitch if form == "v16" else used                              # v16 writes the padding: inside the view; else: moat
    out = Out(B * N, cols, pitch, dev, dtype, lead=out_lead)
    assert out.v.data_ptr() % 256 == out_addr % 256
    L = _L()
    a = (len(segs), _ptrs(srcs), _ptrs([t if t is not None else 0 for t in idxs]), _ints([s["width"] for s in segs]),
         _ints([s["kind"] for s in segs]), _ints([s.get("nsrc", 0) for s in segs]), B, N, _vp(out.v))
    if plain:
        assert pad == 0 and dtype == F32
        rc = L.hsp_concat_rows(*a, _stream())
    else:
        rc = (L.hsp_concat_rows_bf16 if dtype == BF else L.hsp_concat_rows_pitched)(*a, pitch, _stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    assert out.intact(), f"{form}: wrote outside rows x pitch" + ("" if form == "v16" else " or into the padding")
    want = R.concat_ref(segs, B, N)
    assert want.dtype == dtype
    _same_bits(out.v[:, :used], want, f"{form} assembly, B {B} N {N} widths {[s['width'] for s in segs]} pad {pad}")
    if form == "v16" and pad:
        padv = _bits(out.v[:, used:])
        assert not padv.any(), f"v16: {int((padv != 0).sum())} of {padv.numel()} padding elements are not zero (pad {pad})"
    return form


def _v16_segs(B, N, g, dtype, where, special):
    """widths (128, 256, 512) -- kind 0, 1, 0 -- with the kind 2 / 3 segment `special` (width 8) first, in the middle or last"""
    segs = [_seg(0, 128, B, N, g, dtype), _seg(1, 256, B, N, g, dtype, nsrc=7), _seg(0, 512, B, N, g, dtype)]
    sp = _seg(special, 8, B, N, g)
    segs.insert({"first": 0, "middle": 2, "last": 3}[where], sp)
    return segs


@pytest.mark.parametrize("special", [2, 3], ids=["kind2", "kind3"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("pad", [0, 2, 68])
def test_concat_16_byte_form(dev, pad, where, special):
    """fp32 rows of 128 + 256 + 512 + 8 columns: 16-byte chunks at pad 0 and 68 (every padding column zeroed), element pairs at
    pad 2 (a pitch of 906 elements is no multiple of 16 bytes: the padding keeps its sentinel)"""
    B, N = 3, 5
    g = torch.Generator().manual_seed(100 + pad)
    _run_concat(_v16_segs(B, N, g, F32, where, special), B, N, pad, dev, expect="pair" if pad == 2 else "v16", plain=(pad == 0))


@pytest.mark.parametrize("pad", [0, 2, 10, 66, 130])
def test_concat_16_byte_form_pads_after_a_one_hot_of_six(dev, pad):
    """the feat assembly's own layout: a one-hot of 6 columns last, so used = 2 mod 4 and pads of 2, 66, 130 keep the 16-byte form"""
    B, N = 3, 5
    g = torch.Generator().manual_seed(200 + pad)
    segs = [_seg(0, 128, B, N, g), _seg(1, 256, B, N, g, nsrc=4), _seg(3, 6, B, N, g, ids=[0.0, 5.0, 2.7])]
    _run_concat(segs, B, N, pad, dev, expect="v16" if pad % 4 == 2 else "pair")


@pytest.mark.parametrize("pad", [0, 2, 68, 72])
@pytest.mark.parametrize("where", ["first", "last"])
def test_concat_16_byte_form_bf16(dev, pad, where):
    """bf16 rows: 16 bytes are 8 elements -- pads 0 and 72 take the 16-byte form, 2 and 68 element pairs; a kind 2 source equals
    .bfloat16() of the fp32 row"""
    B, N = 3, 5
    g = torch.Generator().manual_seed(300 + pad)
    segs = _v16_segs(B, N, g, BF, where, 2)
    _run_concat(segs, B, N, pad, dev, BF, expect="v16" if pad % 8 == 0 else "pair")
    k2 = next(s for s in segs if s["kind"] == 2)
    c0 = sum(s["width"] for s in segs[:segs.index(k2)])
    assert torch.equal(R.concat_ref(segs, B, N)[:, c0:c0 + 8], k2["src"].bfloat16().repeat_interleave(N, 0))


@pytest.mark.parametrize("dtype,widths", [(F32, (6, 10, 2)), (BF, (4, 12, 2)), (F32, (258, 6)), (BF, (258, 516)), (F32, (516, 2))],
                         ids=["f32", "bf16", "f32-258", "bf16-258-516", "f32-516"])
@pytest.mark.parametrize("pad", [0, 2])
def test_concat_pair_form(dev, dtype, widths, pad):
    B, N = 3, 5
    g = torch.Generator().manual_seed(400 + pad + widths[0])
    segs = [_seg((0, 1, 0)[i % 3], w, B, N, g, dtype, nsrc=3 + i) for i, w in enumerate(widths)]
    _run_concat(segs, B, N, pad, dev, dtype, expect="pair")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["odd-widths", "odd-pitch", "odd-source", "odd-out", "515", "258-odd-source", "v16-but-source-8"])
def test_concat_scalar_and_misaligned_forms(dev, dtype, case):
    """scalars wherever one condition of the pair form fails; a 16-byte layout whose source sits on 8 (bf16: 4) bytes is pairs"""
    B, N = 3, 5
    g = torch.Generator().manual_seed(500)
    lead, pad, expect = LEAD, 0, "scalar"
    if case == "odd-widths":
        segs = [_seg(0, 3, B, N, g, dtype), _seg(1, 5, B, N, g, dtype, nsrc=4)]
    elif case == "odd-pitch":
        segs, pad = [_seg(0, 4, B, N, g, dtype), _seg(1, 4, B, N, g, dtype, nsrc=4)], 1
    elif case == "odd-source":
        segs = [_seg(0, 4, B, N, g, dtype), _seg(1, 4, B, N, g, dtype, nsrc=4, off=1)]
    elif case == "odd-out":
        segs, lead = [_seg(0, 4, B, N, g, dtype), _seg(1, 4, B, N, g, dtype, nsrc=4)], LEAD + 1
    elif case == "515":
        segs = [_seg(0, 515, B, N, g, dtype), _seg(2, 3, B, N, g), _seg(1, 258, B, N, g, dtype, nsrc=4)]
    elif case == "258-odd-source":
        segs = [_seg(0, 258, B, N, g, dtype, off=1), _seg(3, 300, B, N, g, ids=[299.0, 0.0, 256.0])]
    else:
        segs, expect, pad = [_seg(0, 128, B, N, g, dtype), _seg(1, 64, B, N, g, dtype, nsrc=4, off=2)], "pair", 8
    _run_concat(segs, B, N, pad, dev, dtype, out_lead=lead, expect=expect)


@pytest.mark.parametrize("B,N", [(1, 1), (3, 1), (1, 3), (5, 1), (1, 5)])
@pytest.mark.parametrize("form", ["v16", "pair", "scalar"])
def test_concat_few_rows(dev, form, B, N):
    g = torch.Generator().manual_seed(600 + B + N)
    widths = {"v16": (4, 4), "pair": (6, 2), "scalar": (3, 5)}[form]
    segs = [_seg(0, widths[0], B, N, g), _seg(1, widths[1], B, N, g, nsrc=2)]
    _run_concat(segs, B, N, 4 if form == "v16" else 0, dev, expect=form)


@pytest.mark.parametrize("form,dtype", [("v16", F32), ("pair", F32), ("scalar", F32), ("v16", BF), ("pair", BF)])
def test_concat_past_the_grid_cap(dev, form, dtype):
    """one row above what a full grid covers in one pass: 4 x 8192 rows in the 16-byte form, 8192 in the others (width-8 rows)"""
    B = 3
    N = 10925 if form == "v16" else 2731
    assert B * N > (32768 if form == "v16" else 8192)
    g = torch.Generator().manual_seed(700)
    e = 16 // (2 if dtype == BF else 4)
    widths = {"v16": (e, e), "pair": (6, 2), "scalar": (3, 5)}[form]
    segs = [_seg(0, widths[0], B, N, g, dtype), _seg(1, widths[1], B, N, g, dtype, nsrc=777)]
    _run_concat(segs, B, N, e if form == "v16" else 0, dev, dtype, expect=form)


@pytest.mark.parametrize("form", ["v16", "scalar"])
def test_concat_one_hot_ids(dev, form):
    """ids 0 and width - 1; -1, width and 1e9 give an all-zero segment; 2.7 is column 2"""
    ids = [0.0, 7.0, -1.0, 8.0, 1e9, 2.7]
    B, N = len(ids), 3
    g = torch.Generator().manual_seed(800)
    w0 = 4 if form == "v16" else 3
    segs = [_seg(0, w0, B, N, g), _seg(3, 8, B, N, g, ids=ids)]
    _run_concat(segs, B, N, 0, dev, expect=form)
    oh = R.concat_ref(segs, B, N)[:, w0:].view(B, N, 8)
    want = torch.zeros(B, 8)
    want[0, 0] = want[1, 7] = want[5, 2] = 1
    assert torch.equal(oh, want[:, None, :].expand(B, N, 8))


def test_concat_kind1_per_segment_sources(dev):
    """B = 3, three gathered segments whose sources have different row counts"""
    B, N = 3, 40
    g = torch.Generator().manual_seed(900)
    segs = [_seg(1, 8, B, N, g, nsrc=1), _seg(1, 4, B, N, g, nsrc=5), _seg(1, 12, B, N, g, nsrc=64), _seg(0, 4, B, N, g)]
    for s in segs[:3]:
        ix = s["idx"].view(B, N)
        assert ix.min() == 0 and ix.max() == s["nsrc"] - 1 and (s["nsrc"] == 1 or len(ix[0].unique()) < N)
    _run_concat(segs, B, N, 0, dev, expect="v16", plain=True)
    _run_concat(segs, B, N, 3, dev, expect="scalar")


def test_concat_eight_segments_and_nine(dev):
    B, N = 2, 6
    g = torch.Generator().manual_seed(1000)
    segs = [_seg(k, 4, B, N, g, nsrc=3) for k in (0, 1, 2, 3, 0, 1, 0, 1)]
    _run_concat(segs, B, N, 0, dev, expect="v16")
    segs.append(_seg(0, 4, B, N, g))
    srcs = [_at(s["src"], dev) for s in segs]
    idxs = [s["idx"].to(dev) if s["kind"] == 1 else None for s in segs]
    out = Out(B * N, 36, 36, dev)
    a = (_ptrs(srcs), _ptrs([t if t is not None else 0 for t in idxs]), _ints([4] * 9), _ints([s["kind"] for s in segs]), _ints([3] * 9), B, N,
         _vp(out.v))
    L = _L()
    assert L.hsp_concat_rows(9, *a, _stream()) == BAD_ARG and L.hsp_concat_rows_pitched(9, *a, 36, _stream()) == BAD_ARG
    assert L.hsp_concat_rows_pitched(0, *a, 36, _stream()) == BAD_ARG and L.hsp_concat_rows_pitched(8, *a, 31, _stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert out.untouched()


# ======================================================================================================================================
# 4  row gather
# ======================================================================================================================================

def _index(B, Nsrc, Nq, g, shared):
    idx = torch.randint(0, Nsrc, (Nq,) if shared else (B, Nq), generator=g, dtype=I32)
    idx[..., 0] = Nsrc - 1
    idx[..., -1] = 0
    return idx


@pytest.mark.parametrize("shared", [0, 1], ids=["per-cloud", "shared"])
@pytest.mark.parametrize("pad", [0, 1, 6])
@pytest.mark.parametrize("C", [4, 48, 256, 1, 3, 6])
def test_gather_rows_fwd(dev, C, pad, shared):
    B, Nsrc, Nq = 3, 17, 41
    g = torch.Generator().manual_seed(C + pad)
    feat = torch.randn(B, Nsrc, C, generator=g)
    idx = _index(B, Nsrc, Nq, g, shared)
    out = Out(B * Nq, C, C + pad, dev)
    fd, ix = feat.to(dev), idx.to(dev)                                   # (named: alive until the kernel has run)
    rc = _L().hsp_gather_rows_fwd(_vp(fd), _vp(ix), shared, B, Nsrc, Nq, C, _vp(out.v), C + pad, _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    _same_bits(out.v, R.gather_fwd_ref(feat, idx).reshape(B * Nq, C), f"gather fwd C {C} stride {C + pad}")


def test_gather_rows_fwd_past_the_grid_cap(dev):
    B, Nsrc, Nq, C = 2, 300, 5000, 256
    assert B * Nq * (C // 4) > 256 * 8 * 256                             # more units than a full grid of 256-thread workgroups
    g = torch.Generator().manual_seed(11)
    feat = torch.randn(B, Nsrc, C, generator=g)
    idx = _index(B, Nsrc, Nq, g, 0)
    out = Out(B * Nq, C, C + 6, dev)
    fd, ix = feat.to(dev), idx.to(dev)
    rc = _L().hsp_gather_rows_fwd(_vp(fd), _vp(ix), 0, B, Nsrc, Nq, C, _vp(out.v), C + 6, _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    _same_bits(out.v, R.gather_fwd_ref(feat, idx).reshape(B * Nq, C), "gather fwd past the cap")


def _tile_plan(B, Nsrc, C):
    return _L().hsp_scatter_tile_plan(B, Nsrc, C, None)


@pytest.mark.parametrize("shared", [0, 1], ids=["per-cloud", "shared"])
@pytest.mark.parametrize("case", ["C6", "odd-stride", "no-tile"])
def test_gather_rows_bwd_atomic_fallback(dev, case, shared):
    """the three dispatch edges into memset + global atomics; per element within n_m 2^-24 sum|g| of the fp64 sum, rows nobody
    selects exactly zero; cloud 0 (the shared list: every cloud) has a hub row that every query selects"""
    B, Nsrc, Nq, C, stride = {"C6": (3, 50, 300, 6, 6), "odd-stride": (3, 50, 300, 8, 9), "no-tile": (2, 9300, 300, 4, 4)}[case]
    if case == "C6":
        assert C % 4 and _tile_plan(B, Nsrc, C) == 0
    elif case == "odd-stride":
        assert _tile_plan(B, Nsrc, C) != 0 and stride % 2 == 1           # a tile fits; the odd row pitch is what sends it here
    else:
        assert C % 4 == 0 and _tile_plan(B, Nsrc, C) == 0 and _tile_plan(B, Nsrc - 100, C) != 0
    g = torch.Generator().manual_seed(21)
    idx = _index(B, Nsrc, Nq, g, shared)
    hub = Nsrc // 3
    if shared:
        idx[:] = hub
    else:
        idx[0] = hub
    gr = torch.randn(B * Nq, C, generator=g) * 2.0 ** torch.randint(-8, 9, (B * Nq, 1), generator=g)
    gr[::7, 0] = 0                                                       # zeros are skipped by the kernel: the same sum
    out = Out(B * Nsrc, C, C, dev)
    gd, ix = _at(gr, dev, 0, stride), idx.to(dev)
    rc = _L().hsp_gather_rows_bwd(_vp(gd), stride, _vp(ix), shared, B, Nsrc, Nq, C, _vp(out.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    want, T, n = R.gather_bwd_ref(gr.view(B, Nq, C), idx, Nsrc)
    got = out.v.cpu().double().view(B, Nsrc, C)
    assert torch.isfinite(got).all()
    assert n[0, hub] == Nq and (n == 0).any()
    assert not got[(n == 0)[..., None].expand_as(got)].any(), "a row no query selects is not zero"
    err = (got - want).abs()
    tol = n[..., None] * R.U * T
    assert bool((err <= tol).all()), f"worst err / bound {(err / tol.clamp_min(1e-300)).max().item():.3f}"
    pos = T > 0
    RATIOS["gather_rows_bwd atomics (bound n_m)"] = max(RATIOS.get("gather_rows_bwd atomics (bound n_m)", 0.0),
                                                        (err[pos] / (R.U * T[pos])).max().item())


def _lens_map(B, seed):
    """a (B,Nq) row map over Nsrc = 21 rows whose list lengths are 0 .. 17, 100, 0 and 3 (a different row labelling per cloud)"""
    rng = np.random.RandomState(seed)
    lens = list(range(18)) + [100, 0, 3]
    Nsrc, Nq = len(lens), sum(lens)
    idx = np.stack([rng.permutation(np.repeat(rng.permutation(Nsrc), lens)) for _ in range(B)]).astype(np.int32)
    off, edge = R.rev_ref(idx, Nsrc)
    assert {int(v) for v in (off[0, 1:] - off[0, :-1])} == set(lens)
    return idx, off, edge, Nsrc, Nq


def _grad(B, Nq, C, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * Nq, C, generator=g) * 2.0 ** torch.randint(-8, 9, (B * Nq, C), generator=g).float()).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("pad", [0, 2, 6])
@pytest.mark.parametrize("C", [2, 64, 512, 1024, 1028])
def test_gather_rows_bwd_csr(dev, C, pad, dtype):
    """every list length 0 .. 17 and one of 100 (the 8-then-4 walk and its padded last group at every remainder), 1 / 32 / 256 /
    512 / 514 two-element columns, 63 source rows (no multiple of the 256 / 8 / 1 rows of a workgroup), pitch above C"""
    B = 3
    idx, off, edge, Nsrc, Nq = _lens_map(B, 31)
    assert (B * Nsrc) % 8 and (B * Nsrc) % 256
    gr = _grad(B, Nq, C, 32 + C, dtype)
    stride = C + pad
    gd = _at(gr, dev, 0, stride)
    assert _L().hsp_gather_rows_bwd_csr_takes(gr.element_size(), C, stride, gd.data_ptr() % 16) == 1
    out = Out(B * Nsrc, C, C, dev, dtype)
    fn = _L().hsp_gather_rows_bwd_csr_bf16 if dtype == BF else _L().hsp_gather_rows_bwd_csr
    od, ed = torch.from_numpy(off).to(dev), torch.from_numpy(edge).to(dev)
    rc = fn(_vp(gd), stride, _vp(od), _vp(ed), B, Nsrc, Nq, C, _vp(out.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    want = R.gather_bwd_serial(gr.view(B, Nq, C), off, edge, Nsrc)
    _same_bits(out.v, want.view(B * Nsrc, C), f"csr backward C {C} stride {stride}")


def _multi_args(segs, gd, B, Nq, pitch, dev, dtype):
    """segs: [(col0, C, off, edge, Nsrc)] -> (the ctypes arguments, the outputs)"""
    outs = [Out(B * s[4], s[1], s[1], dev, dtype) for s in segs]
    offs = [torch.from_numpy(s[2]).to(dev) for s in segs]
    edges = [torch.from_numpy(s[3]).to(dev) for s in segs]
    eb = gd.element_size()
    a = (len(segs), _ptrs([gd.data_ptr() + s[0] * eb for s in segs]), pitch, _ptrs(offs), _ptrs(edges), B, _ints([s[4] for s in segs]), Nq,
         _ints([s[1] for s in segs]), _ptrs([o.v for o in outs]), _stream())
    return a, outs, (offs, edges)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_gather_rows_bwd_csr_multi(dev, dtype):
    """four segments of one gradient tensor: columns 0 and 196 sit on 16 bytes (bf16: 8) with widths 64 and 32 -- four-element
    columns --, column 64 has width 2 and column 66 sits on 8 bytes (bf16: 4) -- two-element columns; the source row counts
    21, 40, 7, 21 make the launch reorder them (fewest rows first), and the results come back in the caller's order"""
    B = 3
    idx0, off0, edge0, Nsrc0, Nq = _lens_map(B, 41)
    rng = np.random.RandomState(42)
    layout = [(0, 64, Nsrc0), (64, 2, 40), (66, 128, 7), (196, 32, Nsrc0)]
    pitch = 228
    gr = _grad(B, Nq, pitch, 43, dtype)
    gd = _at(gr, dev, 0, pitch)
    eb = gr.element_size()
    segs = []
    for i, (c0, C, ns) in enumerate(layout):
        if i == 0:
            off, edge = off0, edge0
        else:
            off, edge = R.rev_ref(rng.randint(0, ns, size=(B, Nq)), ns)
        segs.append((c0, C, off, edge, ns))
        assert _L().hsp_gather_rows_bwd_csr_takes(eb, C, pitch, (gd.data_ptr() + c0 * eb) % 16) == 1
    vec4 = [C % 4 == 0 and pitch % 4 == 0 and ((gd.data_ptr() + c0 * eb) % (4 * eb)) == 0 for c0, C, _ in layout]
    assert vec4 == [True, False, False, True]
    a, outs, keep = _multi_args(segs, gd, B, Nq, pitch, dev, dtype)
    fn = _L().hsp_gather_rows_bwd_csr_multi_bf16 if dtype == BF else _L().hsp_gather_rows_bwd_csr_multi
    rc = fn(*a)
    torch.cuda.synchronize()
    assert rc == OK
    for (c0, C, off, edge, ns), o in zip(segs, outs):
        assert o.intact()
        want = R.gather_bwd_serial(gr.view(B, Nq, pitch)[:, :, c0:c0 + C].contiguous(), off, edge, ns)
        _same_bits(o.v, want.view(B * ns, C), f"multi segment at column {c0}, C {C}, Nsrc {ns}")


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_gather_rows_bwd_csr_declines_six_columns(dev, dtype):
    B = 3
    idx, off, edge, Nsrc, Nq = _lens_map(B, 51)
    gr = _grad(B, Nq, 14, 52, dtype)
    gd = _at(gr, dev, 0, 14)
    assert _L().hsp_gather_rows_bwd_csr_takes(gr.element_size(), 6, 14, 0) == 0
    out = Out(B * Nsrc, 6, 6, dev, dtype)
    od, ed = torch.from_numpy(off).to(dev), torch.from_numpy(edge).to(dev)
    fn = _L().hsp_gather_rows_bwd_csr_bf16 if dtype == BF else _L().hsp_gather_rows_bwd_csr
    assert fn(_vp(gd), 14, _vp(od), _vp(ed), B, Nsrc, Nq, 6, _vp(out.v), _stream()) == UNSUPPORTED
    a, outs, keep = _multi_args([(0, 8, off, edge, Nsrc), (8, 6, off, edge, Nsrc)], gd, B, Nq, 14, dev, dtype)
    fm = _L().hsp_gather_rows_bwd_csr_multi_bf16 if dtype == BF else _L().hsp_gather_rows_bwd_csr_multi
    assert fm(*a) == UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and all(o.untouched() for o in outs)


# ======================================================================================================================================
# 5  reverse-edge build
# ======================================================================================================================================

def _route(Nsrc, Nq, k):
    return _L().hsp_rev_build_edges_in_lds(Nsrc, Nq, k)


def _rev_lists(B, Nq, Nsrc, k, kstride, seed, mode="random"):
    """idx (B,Nq,kstride) int32, every entry in [0, Nsrc) (the columns past k too, which nobody reads)"""
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, Nsrc, size=(B, Nq, kstride)).astype(np.int32)
    if mode == "hub":
        idx[:, :, :k] = Nsrc // 2
    elif mode == "few":                                                  # three busy rows: long lists, filled by whole chunks
        idx[:, :, :k] = rng.randint(0, min(3, Nsrc), size=(B, Nq, k)) * (Nsrc // 3 if Nsrc >= 3 else 0)
    elif mode == "shuffled":                                             # a permutation-like row map, rows 0 and Nsrc - 1 hit
        for b in range(B):
            idx[b, :, 0] = rng.permutation(np.arange(Nq) % Nsrc)
    if mode == "random" and Nq * k >= 2:
        idx[:, 0, 0] = Nsrc - 1
        idx[:, -1, k - 1] = 0
    return idx


def _rev_outputs(B, Nq, Nsrc, k, dev):
    return Out(B, Nsrc + 1, Nsrc + 1, dev, I32), Out(B, Nq * k, Nq * k, dev, I32)


def _hold_rev(off, edge, idx, k, Nsrc, what, qsel=None):
    assert off.intact() and edge.intact(), f"{what}: wrote outside rev_off / rev_edge"
    woff, wedge = R.rev_ref(R.rev_targets(idx, k, qsel), Nsrc)
    _same_bits(off.v, torch.from_numpy(woff), f"{what}: rev_off")
    _same_bits(edge.v, torch.from_numpy(wedge), f"{what}: rev_edge")


REV_CASES = [
    # B, Nq, Nsrc, k, kstride, mode, edges in LDS
    (1, 1700, 1700, 20, 20, "random", 1), (1, 1792, 1792, 20, 20, "random", 0), (3, 1700, 1700, 20, 23, "random", 1),
    (3, 1792, 1792, 20, 20, "random", 0),
    (3, 40, 1, 4, 4, "random", 1), (3, 200, 63, 4, 4, "random", 1), (1, 600, 1023, 3, 3, "random", 1), (3, 600, 1024, 3, 5, "random", 1),
    (3, 600, 1025, 3, 3, "random", 1), (1, 900, 2049, 5, 5, "random", 1), (3, 50, 35839, 4, 4, "random", 0), (1, 50, 35839, 4, 6, "random", 0),
    (3, 1, 5, 1, 1, "random", 1), (3, 341, 100, 3, 3, "random", 1), (3, 256, 100, 4, 4, "random", 1), (3, 205, 100, 5, 7, "random", 1),
    (3, 1024, 3, 4, 4, "few", 1), (1, 1025, 7, 2, 2, "few", 1),
    (3, 1025, 300, 1, 1, "shuffled", 1), (3, 1023, 64, 1, 3, "shuffled", 1), (3, 1024, 2049, 1, 1, "shuffled", 1),
    (3, 1025, 64, 1, 1, "hub", 1), (3, 300, 1, 1, 1, "random", 1), (1, 5000, 1024, 1, 1, "random", 1),
]


@pytest.mark.parametrize("B,Nq,Nsrc,k,kstride,mode,in_lds", REV_CASES)
def test_rev_build_whole_index(dev, B, Nq, Nsrc, k, kstride, mode, in_lds):
    """the whole of rev_off and rev_edge, every row.  The order in which a chunk's 1024 edges land in a list is the order of the
    kernel's LDS atomics, which no input dictates: the "few" cases give the per-row sort the shape where that order matters most
    (three busy rows, every chunk adds hundreds of edges to each list), the rest Nsrc around the scan's multiples of 1024, the
    histogram limit 35839, E around a chunk, kstride > k and the k = 1 rank path (shuffled, a hub, one source row)."""
    assert _route(Nsrc, Nq, k) == in_lds                                 # the form this case enters
    idx = _rev_lists(B, Nq, Nsrc, k, kstride, 61 + Nq + Nsrc, mode)
    off, edge = _rev_outputs(B, Nq, Nsrc, k, dev)
    ix = torch.from_numpy(idx).to(dev)
    rc = _L().hsp_rev_build(_vp(ix), B, Nq, Nsrc, k, kstride, _vp(off.v), _vp(edge.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK
    _hold_rev(off, edge, idx, k, Nsrc, f"rev_build ({B},{Nq},{Nsrc},{k},{kstride}) {mode}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per_cloud", [0, 1], ids=["shared", "per-cloud"])
@pytest.mark.parametrize("Nidx,Nq,Nsrc,k,kstride,in_lds", [(100, 37, 60, 4, 4, 1), (100, 260, 60, 4, 6, 1), (2000, 1792, 2000, 20, 20, 0),
                                                             (50, 1025, 9, 1, 1, 1)])
def test_rev_build_sel(dev, B, per_cloud, Nidx, Nq, Nsrc, k, kstride, in_lds):
    """the kept rows' lists: Nq != Nidx, rows named more than once (Nq > Nidx names every row at least twice)"""
    assert _route(Nsrc, Nq, k) == in_lds
    idx = _rev_lists(B, Nidx, Nsrc, k, kstride, 71 + Nq)
    rng = np.random.RandomState(72 + Nq)
    qsel = rng.randint(0, Nidx, size=(B, Nq) if per_cloud else (Nq,)).astype(np.int32)
    qsel[..., 0], qsel[..., 1], qsel[..., -1] = Nidx - 1, Nidx - 1, 0
    off, edge = _rev_outputs(B, Nq, Nsrc, k, dev)
    ix, qs = torch.from_numpy(idx).to(dev), torch.from_numpy(qsel).to(dev)
    rc = _L().hsp_rev_build_sel(_vp(ix), _vp(qs), Nq if per_cloud else 0, B, Nidx, Nq, Nsrc, k, kstride, _vp(off.v), _vp(edge.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK
    _hold_rev(off, edge, idx, k, Nsrc, f"rev_build_sel ({B},{Nidx},{Nq},{Nsrc},{k})", qsel)


@pytest.mark.parametrize("B", [1, 3])
def test_rev_build_multi(dev, B):
    """four maps of different (Nq, Nsrc, k) in one launch, one of them with its edges in global memory"""
    maps = [(300, 64, 1, 1), (1792, 1792, 20, 20), (205, 1025, 5, 7), (1700, 1700, 20, 20)]
    assert [_route(ns, nq, k) for nq, ns, k, _ in maps] == [1, 0, 1, 1]
    idxs = [_rev_lists(B, nq, ns, k, ks, 81 + i) for i, (nq, ns, k, ks) in enumerate(maps)]
    dev_idx = [torch.from_numpy(i).to(dev) for i in idxs]
    outs = [_rev_outputs(B, nq, ns, k, dev) for nq, ns, k, _ in maps]
    rc = _L().hsp_rev_build_multi(4, _ptrs(dev_idx), B, _ints([m[0] for m in maps]), _ints([m[1] for m in maps]), _ints([m[2] for m in maps]),
                                  _ints([m[3] for m in maps]), _ptrs([o[0].v for o in outs]), _ptrs([o[1].v for o in outs]), _stream())
    torch.cuda.synchronize()
    assert rc == OK
    for (nq, ns, k, ks), idx, (off, edge) in zip(maps, idxs, outs):
        _hold_rev(off, edge, idx, k, ns, f"rev_build_multi map ({nq},{ns},{k},{ks})")


def test_rev_build_declines_write_nothing(dev):
    B, Nq, Nsrc, k = 2, 10, 35840, 2
    assert _route(Nsrc, Nq, k) == -1
    idx = torch.from_numpy(_rev_lists(B, Nq, Nsrc, k, k, 91)).to(dev)
    off, edge = _rev_outputs(B, Nq, Nsrc, k, dev)
    L = _L()
    assert L.hsp_rev_build(_vp(idx), B, Nq, Nsrc, k, k, _vp(off.v), _vp(edge.v), _stream()) == UNSUPPORTED
    assert L.hsp_rev_build(_vp(idx), B, Nq, 100, k, k - 1, _vp(off.v), _vp(edge.v), _stream()) == BAD_ARG
    qs = torch.zeros(Nq, dtype=I32, device=dev)
    assert L.hsp_rev_build_sel(_vp(idx), _vp(qs), 0, B, Nq, Nq, Nsrc, k, k, _vp(off.v), _vp(edge.v), _stream()) == UNSUPPORTED
    assert L.hsp_rev_build_sel(_vp(idx), _vp(qs), Nq - 1, B, Nq, Nq, 100, k, k, _vp(off.v), _vp(edge.v), _stream()) == BAD_ARG
    assert L.hsp_rev_build_multi(1, _ptrs([idx]), B, _ints([Nq]), _ints([Nsrc]), _ints([k]), _ints([k]), _ptrs([off.v]), _ptrs([edge.v]),
                                 _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert off.untouched() and edge.untouched()


# ======================================================================================================================================
# 6  the two fused passes
# ======================================================================================================================================

@pytest.mark.parametrize("B,N,C", [(3, 37, 4), (3, 37, 12), (3, 5, 1024), (3, 1, 12), (1, 1, 4), (3, 700, 1024)])
def test_residual_bias(dev, B, N, C):
    """out + (f + t[b]) in fp32, bit for bit; (3, 700, 1024) is more float4 units than a full grid covers in one pass"""
    if N == 700:
        assert B * N * (C // 4) > 256 * 8 * 256
    g = torch.Generator().manual_seed(C + N)
    o = torch.randn(B, N, C, generator=g)
    f = torch.randn(B, N, C, generator=g) * 2.0 ** torch.randint(-6, 7, (B, N, C), generator=g).float()
    t = torch.randn(B, C, generator=g) * 2.0 ** torch.randint(-6, 7, (B, C), generator=g).float()
    out = Out(B * N, C, C, dev, init=o.view(B * N, C))
    fd, td = f.to(dev), t.to(dev)
    rc = _L().hsp_residual_bias(_vp(out.v), _vp(fd), _vp(td), B, N, C, _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    want = R.residual_bias_ref(o.numpy(), f.numpy(), t.numpy())
    if B * N * C >= 200:
        assert not np.array_equal(want, ((o + f) + t[:, None, :]).numpy())   # the data tell the two associations apart
    _same_bits(out.v, torch.from_numpy(want).view(B * N, C), f"residual_bias ({B},{N},{C})")


def test_residual_bias_declines_six_columns(dev):
    B, N, C = 3, 7, 6
    g = torch.Generator().manual_seed(6)
    out = Out(B * N, C, C, dev, init=torch.randn(B * N, C, generator=g))
    fd, td = torch.randn(B, N, C, generator=g).to(dev), torch.randn(B, C, generator=g).to(dev)
    rc = _L().hsp_residual_bias(_vp(out.v), _vp(fd), _vp(td), B, N, C, _stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and out.untouched()


def _relu_case(Rn, C, seed):
    g = torch.Generator().manual_seed(seed)
    ga, gb = torch.randn(Rn, C, generator=g), torch.randn(Rn, C, generator=g)
    y = torch.randn(Rn, C, generator=g)
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, 2.0 ** -140, -2.0 ** -140, 2.0 ** -149, -2.0 ** -126])
    pick = torch.randint(0, 4 * len(special), (Rn, C), generator=g)
    y = torch.where(pick < len(special), special[pick.clamp_max(len(special) - 1)], y)
    if Rn * C >= 200:
        assert (y == 0).any() and ((y > 0) & (y < 2.0 ** -126)).any() and (y == 2.0 ** -126).any()
    return ga, gb, y


@pytest.mark.parametrize("Rn,C,pa,pb,with_gb", [(37, 6, 0, 0, 1), (37, 6, 2, 4, 1), (37, 6, 2, 0, 0), (5, 1286, 2, 0, 1), (1, 2, 0, 0, 1),
                                                (2100, 512, 0, 6, 1)])
def test_add_relu_bwd(dev, Rn, C, pa, pb, with_gb):
    """(ga + gb) * [y > 0] bit for bit; y holds +0, -0, the smallest positive normal and positive / negative subnormals (a positive
    subnormal passes the gradient, as threshold_backward); (2100, 512) is more pairs than a full grid covers in one pass"""
    if Rn == 2100:
        assert Rn * (C // 2) > 256 * 8 * 256
    ga, gb, y = _relu_case(Rn, C, Rn + C)
    out = Out(Rn, C, C, dev)
    gbd = _at(gb, dev, 0, C + pb) if with_gb else None
    gad, yd = _at(ga, dev, 0, C + pa), y.to(dev)
    rc = _L().hsp_add_relu_bwd(_vp(gad), C + pa, _vp(gbd), C + pb if with_gb else 0, _vp(yd), Rn, C, _vp(out.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    want = torch.from_numpy(R.add_relu_bwd_ref(ga.numpy(), gb.numpy() if with_gb else None, y.numpy()))
    _same_bits(out.v, want, f"add_relu_bwd ({Rn},{C}) lda {C + pa} ldb {C + pb}")
    ref = torch.ops.aten.threshold_backward(ga + gb if with_gb else ga, y, 0.0)
    assert torch.equal(want, ref)                                        # no NaN among y: autograd's own mask


def test_add_relu_bwd_nan_activation_gives_zero(dev):
    """include/hsp.h: y = NaN fails the comparison y > 0, the gradient is dropped (threshold_backward would pass it)"""
    ga, gb, y = _relu_case(9, 8, 5)
    y[::2, ::3] = NAN
    out = Out(9, 8, 8, dev)
    gad, gbd, yd = ga.to(dev), gb.to(dev), y.to(dev)
    rc = _L().hsp_add_relu_bwd(_vp(gad), 8, _vp(gbd), 8, _vp(yd), 9, 8, _vp(out.v), _stream())
    torch.cuda.synchronize()
    assert rc == OK and out.intact()
    got = out.v.cpu()
    assert not got[torch.isnan(y)].any() and not torch.signbit(got[torch.isnan(y)]).any()
    _same_bits(got, torch.from_numpy(R.add_relu_bwd_ref(ga.numpy(), gb.numpy(), y.numpy())), "add_relu_bwd with NaN activations")
    assert torch.ops.aten.threshold_backward(ga + gb, y, 0.0)[torch.isnan(y)].ne(0).all()


@pytest.mark.parametrize("case", ["odd-ldb", "odd-lda", "odd-C", "gb-on-4-bytes"])
def test_add_relu_bwd_declines(dev, case):
    Rn, C = 5, 6
    ga, gb, y = _relu_case(Rn, 8, 7)
    lda, ldb, off = 8, 8, 0
    if case == "odd-ldb":
        ldb = 7
    elif case == "odd-lda":
        lda = 7
    elif case == "odd-C":
        C = 5
    else:
        off = 1
    out = Out(Rn, C, C, dev)
    gad, gbd, yd = _at(ga, dev), _at(gb, dev, off), y[:, :C].contiguous().to(dev)
    rc = _L().hsp_add_relu_bwd(_vp(gad), lda, _vp(gbd), ldb, _vp(yd), Rn, C, _vp(out.v), _stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and out.untouched()


# ======================================================================================================================================

def test_zz_measured_ratios():
    """recorded, not asserted: the worst err / (2^-24 sum|t|) of every form over this file's cases (docstring)"""
    for k in sorted(RATIOS):
        print(f"measured ratio  {k:42s} {RATIOS[k]:.3f}")
