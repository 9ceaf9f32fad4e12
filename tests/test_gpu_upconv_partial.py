"""GPU (-m gpu): gn_upconv_partial (csrc/upconv.hip), the producer of the polyphase partial, held to fp64 by itself -- per parity class, on every branch
and tail of both kernel templates -- and not through the sum the layer test sees three launches downstream.

The definition is tests/upconv_reference.py's partial_reference (fp64 on the CPU: affine, nearest upsampling, a 3x3x3 convolution zero-padded at the
fine border, de-interleaved; no polyphase_weights, no pack).  Inputs from its seeded generator (exact zeros and -0.0 in x1, sample 1 of a batched case
2^10 above the others), a1 / d1 from ops.groupnorm_affine on the real statistics of x1 (gamma = rand + 0.5, beta = randn + 1: d far from zero).

Which case runs which branch (upconv_partial_kernel<NT, F16>: <1, *> for Cout % 64 != 0, two coarse z-slices per workgroup; <2, *> otherwise, one;
F16 = true in mode f16x2, false in bf16x2 -- every case runs both; nblk = gridDim.x, what the XCD remap of blockIdx.x sees):
    (1, 1, 1)   16 -> 32 / 64   <1> / <2>, nblk 1: every halo voxel but one is padding; masked epilogue; single slice (nsteps = 8: both prefetches end at once)
    (2, 8, 8)   32 -> 32        <1>, nblk 1: one whole tile, the uniform-address epilogue
    (1, 8, 8)   32 -> 64        <2>, nblk 1: one whole tile, the uniform-address epilogue
    (3, 9, 5)   48 -> 32, B 3   <1>, nblk 4 (rx = 4): ragged on all axes, odd Dc (the gz < Dc tail of the second z-slice), 3 slices (odd), batch
    (3, 9, 5)   48 -> 96        <1>, ncb = 3, nblk 12 (qx = 1, rx = 4)
    (3, 9, 5)   16 -> 64, B 3   <2>, nblk 6: ragged, single slice, batch
    (3, 9, 5)   32 -> 192       <2>, ncb = 3, nblk 18 (qx = 2, rx = 2)
    (2, 3, 5)   384 -> 128      <2>, ncb = 2, nblk 4: the full a / d table, 24 slices
    (5, 10, 17) 32 -> 64, B 2   <2>, nblk 30: several tiles per axis, whole and masked tiles in one launch, tails in y and x
    (4, 8, 16)  16 -> 64        <2>, nblk 8 (rx = 0)
    (16, 8, 8)  16 -> 32        <1>, nblk 8 (rx = 0)
Every case in f16x2 with act_inv from groupnorm_affine(with_act_scale=True) and in bf16x2 with act_inv = None; the (3, 9, 5) cases in f16x2 with
act_inv = None as well (act_inv == NULL together with fp16 planes).  test_upconv_reference_host.py proves on the CPU that the table holds each of
the four kinds of grid for each template and that the restated remap is a bijection.

What a case asserts, both packs (ops.pack_upconv_weight of polyphase_weights, ops.pack_upconv_weight_device) and torch.equal between the two:
  (b) every element written, nothing else: the entry on a NaN-prefilled buffer between 8 guard rows of 7.25 -- no NaN left, guards untouched, the
      inside torch.equal to what ops.upconv_partial returned (which allocates with torch.empty).  A remap or tail error fails here;
  (c) sample b of the batched launch torch.equal to the B = 1 launch of that sample; two runs torch.equal (no atomics in this kernel);
  (a) the largest error of each of the 8 parity classes against fp64.  The bar is never the code under test: the upsampled source is materialised at
      full resolution and run as a ONE-source layer (same a1, d1, relu off) through the project's literal kernels -- f16x2: 2 * max(e32, 2e-6), e32 the
      error of ops.conv3d_gcr (fp32 MFMA); bf16x2: 2 * max(e_lit, 2e-6), e_lit the error of ops.conv3d_gcr_split in mode 2, and never above
      2e-4 * max(1, max|ref|) (test_conv3d_split_against_torch's bar for two bf16 planes);
  (d) the (3, 9, 5) cases: the result is more than 100 bars away from padding_before_affine at some border voxel.
Further: the range contract of the product path (gamma x 1e-4, 1, 1e4); weight rows (a x1000 row and a x1000 weight: per (class, row) relative
error, the scale the pack keeps per (class, row); an all-zero row: exactly 0.0 in its 8 classes; a row whose merged taps cancel to 0 on the host);
the refusals of the entry (by message, a guarded buffer unchanged) and of the wrapper (by name, before any launch).

NOT covered: grids of more than 64 workgroups (shapes above the table are out of scope; the remap's restatement is proved a bijection to 64 on the
CPU); a source whose byte offsets pass 2^31 (cannot be small); non-finite inputs.

Exchanging two tap products was tried once, on a scratch build never committed: in upconv_partial_kernel the A-fragment offset of the next tap
with iy and ix exchanged (taps 1 <-> 2 and 5 <-> 6 read each other's halo voxels, the B fragments stay).  All 28 runs of
test_partial_against_fp64_per_class failed at the same named assertion, `assert errs[c] <= bar, ("(a) against fp64", ...)`, in class 0 (class 1 at
(1, 1, 1)) with errors of 2.1 ... 5.2 against bars of 4e-6 ... 8e-5; the range contract, the outlier rows and the zero / cancelling rows failed too; only
the two refusal tests passed.  (b) and (c) held, as they should: that mutation moves no store and is the same in every launch.  Dropping the `gz < p.Dc`
guard was NOT run: at (3, 9, 5) under <1> it stores the 45 rows of a z-slice past the end of the last sample (and into the next sample's first slice),
through the 8 guard rows and beyond -- an out-of-bounds write is not something to run; by reading, (b)'s `a write outside the partial` is what it hits.

Figures of one run on an MI355X (the `[upconv-partial]` lines: the largest error against fp64 over the 8 parity classes [smallest class ... largest
class], the class that holds it, the yardstick's error on the same quantity and the bar).  Both packs gave the same bits in every run.
    case                    f16x2, act_inv                            f16x2, act_inv NULL        bf16x2 (cap 2e-4 * max|ref| = 4.9e-4 ... 1.5e-3)
    (1,1,1) 16->32          1.5e-07 .. 3.00e-07 cls 0 (e32 1.02e-06, bar 4.00e-06)               6.0e-06 .. 1.67e-05 cls 2 (e_lit 1.54e-05, bar 3.09e-05)
    (1,1,1) 16->64          1.7e-07 .. 3.19e-07 cls 7 (e32 8.53e-07, bar 4.00e-06)               7.3e-06 .. 1.66e-05 cls 4 (e_lit 1.15e-05, bar 2.30e-05)
    (2,8,8) 32->32          9.2e-07 .. 1.60e-06 cls 7 (e32 4.25e-06, bar 8.50e-06)               2.4e-05 .. 3.41e-05 cls 3 (e_lit 3.07e-05, bar 6.14e-05)
    (1,8,8) 32->64          7.5e-07 .. 1.26e-06 cls 6 (e32 2.94e-06, bar 5.89e-06)               2.6e-05 .. 3.65e-05 cls 2 (e_lit 2.78e-05, bar 5.55e-05)
    (3,9,5) 48->32 B3       1.1e-06 .. 1.90e-06 cls 4 (e32 4.05e-06, bar 8.11e-06)   1.90e-06 cls 4   3.0e-05 .. 4.05e-05 cls 6 (e_lit 3.34e-05, bar 6.68e-05)
    (3,9,5) 48->96          1.2e-06 .. 1.52e-06 cls 6 (e32 5.13e-06, bar 1.03e-05)   1.52e-06 cls 6   3.0e-05 .. 3.61e-05 cls 1 (e_lit 3.47e-05, bar 6.95e-05)
    (3,9,5) 16->64 B3       1.5e-06 .. 2.40e-06 cls 7 (e32 5.88e-06, bar 1.18e-05)   2.40e-06 cls 7   3.3e-05 .. 4.04e-05 cls 1 (e_lit 3.74e-05, bar 7.49e-05)
    (3,9,5) 32->192         1.2e-06 .. 1.90e-06 cls 6 (e32 4.51e-06, bar 9.01e-06)   2.13e-06 cls 6   3.0e-05 .. 3.90e-05 cls 0 (e_lit 3.46e-05, bar 6.93e-05)
    (2,3,5) 384->128        1.0e-06 .. 1.60e-06 cls 7 (e32 2.74e-06, bar 5.47e-06)               2.1e-05 .. 2.80e-05 cls 3 (e_lit 2.83e-05, bar 5.65e-05)
    (5,10,17) 32->64 B2     1.4e-06 .. 2.17e-06 cls 4 (e32 5.59e-06, bar 1.12e-05)               3.4e-05 .. 4.38e-05 cls 3 (e_lit 4.03e-05, bar 8.06e-05)
    (4,8,16) 16->64         1.5e-06 .. 2.50e-06 cls 4 (e32 6.50e-06, bar 1.30e-05)               3.3e-05 .. 4.55e-05 cls 1 (e_lit 3.56e-05, bar 7.12e-05)
    (16,8,8) 16->32         1.5e-06 .. 2.35e-06 cls 2 (e32 6.45e-06, bar 1.29e-05)               3.4e-05 .. 4.00e-05 cls 4 (e_lit 3.60e-05, bar 7.19e-05)
max|ref| 2.5 ... 7.6.  No class stands out: the largest error moves between classes from case to case, and the two-plane kernel is 1.7 ... 3.4 times
closer to fp64 than the fp32-MFMA yardstick in f16x2 and level with the literal mode-2 kernel in bf16x2.
    range contract   gamma x 1e-4 / 1 / 1e4: err / max|ref| 3.44e-07 / 2.77e-07 / 2.40e-07 (bar 2e-6), activation scales 2^-1 / 2^-1 / 2^-13
    outlier rows     per-(class, row) relative error 6.24e-07 (fp32-MFMA kernel 1.23e-06: bar 2.46e-06), both packs
    zero / cancelling rows   class errors 1.05e-06 ... 1.90e-06, bar 8.11e-06; the zero row exactly 0.0 in all 8 classes
The module takes about 3 s, the slowest case 0.6 s (the first launch of the session).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import upconv_reference as R  # noqa: E402
from garmentnets_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
F16X2, BF16X2, BF16X3 = ops.SPLIT_F16X2, ops.SPLIT_BF16X2, ops.SPLIT_BF16X3
MODE_NAME = {F16X2: "f16x2", BF16X2: "bf16x2"}
PAD, GUARD = 8, 7.25
RAGGED = (3, 9, 5)
RAGGED_NARROW = next(c for c in R.CASES if c[0] == RAGGED and c[1:] == (48, 32, 3))       # <1>: 48 -> 32, B = 3


# ---------------------------------------------------------------------------------------------------- inputs, references and yardsticks, made once
class _Setup:
    """one case on the host (x1, w, w1, gamma, beta) and on the device (g*); its statistics; the affine without (a0, d0) and with the sample's
    power-of-two activation scale folded in (a2, d2, inv); the upsampled source at full resolution (fine)"""


def _upsample(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).contiguous()


@functools.lru_cache(maxsize=None)
def _setup(case):
    s = _Setup()
    s.case = case
    s.dims, s.C1, s.Cout, s.B = case
    for k, v in R.make_inputs(case).items():
        setattr(s, k, v)
        setattr(s, "g" + k, v.to(DEV).contiguous())
    s.stats = ops.channel_stats(s.gx1)
    s.a0, s.d0 = ops.groupnorm_affine(s.stats, None, R.GROUPS, R.EPS, s.ggamma, s.gbeta)
    s.a2, s.d2, s.inv = ops.groupnorm_affine(s.stats, None, R.GROUPS, R.EPS, s.ggamma, s.gbeta, with_act_scale=True)
    # the affine is GroupNorm's, from the real statistics (the device rows are what every launch and the reference below read)
    a_ref, d_ref = R.affine_reference(s.x1, s.gamma, s.beta)
    for got, want in ((s.a0, a_ref), (s.d0, d_ref), (s.a2 * s.inv[:, None], a_ref), (s.d2 * s.inv[:, None], d_ref)):
        assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max()), case
    s.fine = _upsample(s.gx1)
    return s


def _affine(s, act):
    """-> (a, d, act_inv) as launched and (a, d) in true units: what the reference and the yardsticks read (the scale is a power of two: exact to undo)"""
    if not act:
        return s.a0, s.d0, None, s.a0, s.d0
    return s.a2, s.d2, s.inv, (s.a2 * s.inv[:, None]).contiguous(), (s.d2 * s.inv[:, None]).contiguous()


_REFS = {}


def _reference(x1, a_true, d_true, w1):
    """partial_reference on the device's own affine rows, computed once per distinct input and left unchanged"""
    key = (x1.data_ptr(), w1.data_ptr(), a_true.cpu().numpy().tobytes(), d_true.cpu().numpy().tobytes())
    if key not in _REFS:
        _REFS[key] = (R.partial_reference(x1, a_true.cpu(), d_true.cpu(), w1), x1, w1)        # (the tensors kept alive: their addresses are the key)
    return _REFS[key][0]


@functools.lru_cache(maxsize=None)
def _packs(case, mode):
    s = _setup(case)
    return _both_packs(s.w, s.gw, s.Cout, mode)


def _both_packs(w, gw, cout, mode):
    """-> (the host pack on the device, the device pack) of the raw layer weight"""
    return ops.pack_upconv_weight(ops.polyphase_weights(w, R.C0)[1], cout, mode).to(DEV), ops.pack_upconv_weight_device(gw, R.C0, mode)


def _yardstick(s, w1, a_true, d_true, mode):
    """the project's literal kernel on the SAME quantity: the upsampled source as one full-resolution source, relu off, de-interleaved
    -> [B][Dc][Hc][Wc][8 * Cout] on the host (f16x2: the fp32-MFMA kernel; bf16x2: the split kernel in mode 2)"""
    if mode == F16X2:
        out = ops.conv3d_gcr(s.fine, None, a_true, d_true, ops.pack_conv_weight(w1).to(DEV), s.Cout, relu=False)
    else:
        out = ops.conv3d_gcr_split(s.fine, None, a_true, d_true, ops.pack_conv_weight_split(w1, BF16X2).to(DEV), s.Cout, relu=False)
    return R.deinterleave(out.cpu().double())


@functools.lru_cache(maxsize=None)
def _yardstick_error(case, act, mode):
    s = _setup(case)
    _, _, _, at, dt = _affine(s, act)
    return float((_yardstick(s, s.w1, at, dt, mode) - _reference(s.x1, at, dt, s.w1)).abs().max())


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_inputs():
    yield
    for f in (_setup, _packs, _yardstick_error):
        f.cache_clear()
    _REFS.clear()


def _entry(src1, C1, a, d, wp, mode, out_scale, act_inv, B, Dc, Hc, Wc, Cout, partial):
    return _lib.call("gn_upconv_partial", ops._p(src1), C1, ops._p(a), ops._p(d), ops._p(wp), mode, ops._p(out_scale), ops._p(act_inv), B, Dc, Hc, Wc, Cout,
                     ops._p(partial), ops._stream())


def _guarded(rows, width, inside=float("nan")):
    buf = torch.full((rows + 2 * PAD, width), inside, dtype=torch.float32, device=DEV)
    buf[:PAD] = GUARD
    buf[PAD + rows:] = GUARD
    return buf


def _guards_untouched(buf, rows):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + rows:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------- the cases
RUNS = [(c, F16X2, True) for c in R.CASES] + [(c, BF16X2, False) for c in R.CASES] + [(c, F16X2, False) for c in R.CASES if c[0] == RAGGED]


def _run_id(run):
    case, mode, act = run
    return f"{R.case_id(case)}-{MODE_NAME[mode]}-{'act' if act else 'noact'}"


@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_partial_against_fp64_per_class(run):
    """(a) - (d) of the module docstring for one (case, mode, act_inv)"""
    case, mode, act = run
    s = _setup(case)
    (Dc, Hc, Wc), C1, Cout, B = case
    a, d, inv, at, dt = _affine(s, act)
    host, dev = _packs(case, mode)
    got = ops.upconv_partial(s.gx1, a, d, host, Cout, act_inv=inv)
    assert got.shape == (B, Dc, Hc, Wc, 8 * Cout)
    assert torch.equal(got, ops.upconv_partial(s.gx1, a, d, dev, Cout, act_inv=inv)), "the host pack against the device pack"
    # (b) every element written, nothing else
    rows = B * Dc * Hc * Wc
    buf = _guarded(rows, 8 * Cout)
    _entry(s.gx1, C1, a, d, host.tensor, host.mode, host.out_scale, inv, B, Dc, Hc, Wc, Cout, buf[PAD:])
    inside = buf[PAD:PAD + rows]
    holes = torch.isnan(inside)
    assert not bool(holes.any()), ("(b) elements left unwritten", int(holes.sum()), torch.nonzero(holes.view(B, Dc, Hc, Wc, 8, Cout))[:4].tolist())
    assert _guards_untouched(buf, rows), "(b) a write outside the partial"
    assert torch.equal(inside.view_as(got), got), "(b) the entry on a prefilled buffer against ops.upconv_partial"
    # (c) run to run, and sample b against the B = 1 launch of that sample alone
    assert torch.equal(got, ops.upconv_partial(s.gx1, a, d, host, Cout, act_inv=inv)), "(c) run to run"
    if B > 1:
        for b in range(B):
            one = ops.upconv_partial(s.gx1[b:b + 1], a[b:b + 1], d[b:b + 1], host, Cout, act_inv=None if inv is None else inv[b:b + 1])
            assert torch.equal(got[b], one[0]), ("(c) batch slot against the B = 1 launch", b)
    # (a) against fp64, per parity class
    ref = _reference(s.x1, at, dt, s.w1)
    top = float(ref.abs().max())
    errs = R.class_errors(got.cpu(), ref, Cout)
    worst = max(range(8), key=lambda c: errs[c])
    e_yard = _yardstick_error(case, act, mode)
    bar = 2 * max(e_yard, 2e-6)
    cap = 2e-4 * max(1.0, top) if mode == BF16X2 else float("inf")
    print(f"[upconv-partial] {_run_id(run)}: class errors [{', '.join(f'{e:.2e}' for e in errs)}], largest in class {worst}; "
          f"{'conv3d_gcr' if mode == F16X2 else 'conv3d_gcr_split mode 2'} {e_yard:.2e}, bar {bar:.2e}" + (f", cap {cap:.2e}" if mode == BF16X2 else "")
          + f"; max|ref| {top:.2f}")
    assert torch.isfinite(got).all()
    for c in range(8):
        assert errs[c] <= bar, ("(a) against fp64", _run_id(run), "class", c, errs[c], bar)
        assert errs[c] <= cap, ("(a) the two-bf16-plane bar", _run_id(run), "class", c, errs[c], cap)
    # (d) the zero padding comes after the affine
    if case[0] == RAGGED:
        wrong = R.padding_before_affine(s.x1, at.cpu(), dt.cpu(), s.w1)
        diff = (got.cpu().double() - wrong).abs()
        border = float(diff.max())
        assert float(diff[:, 1:-1, 1:-1, 1:-1].max()) <= bar and border > 100 * bar, ("(d) the padding", border, bar)


def test_product_path_range_contract():
    """gains 1e-4, 1, 1e4 on gamma at (3, 9, 5), 48 -> 32, f16x2 with the sample's activation scale: finite and within 2e-6 * max|ref|
    (test_conv3d_f16x2_range_contract's bar)"""
    case = RAGGED_NARROW
    s = _setup(case)
    for gain in (1.0e-4, 1.0, 1.0e4):
        a, d, inv = ops.groupnorm_affine(s.stats, None, R.GROUPS, R.EPS, s.ggamma * gain, s.gbeta, with_act_scale=True)
        m = torch.log2(inv).cpu()
        assert torch.equal(m, m.round())                                      # exact powers of two
        at, dt = (a * inv[:, None]).contiguous(), (d * inv[:, None]).contiguous()
        ref = _reference(s.x1, at, dt, s.w1)
        scale = float(ref.abs().max())
        outs = [ops.upconv_partial(s.gx1, a, d, pk, s.Cout, act_inv=inv) for pk in _packs(case, F16X2)]
        assert torch.equal(outs[0], outs[1])
        err = float((outs[0].cpu().double() - ref).abs().max())
        print(f"[upconv-partial] range contract gain {gain:g}: act scale 2^{[-int(v) for v in m.tolist()]}, err / max|ref| {err / scale:.2e} (max|ref| {scale:.3g})")
        assert bool(torch.isfinite(outs[0]).all()) and err <= 2e-6 * scale


def _rows_case(w):
    """the (3, 9, 5), 48 -> 32, B = 3 case with another layer weight, f16x2 with the activation scale -> (s, both results, ref, the fp32-MFMA yardstick)"""
    s = _setup(RAGGED_NARROW)
    a, d, inv, at, dt = _affine(s, True)
    w1 = w[:, R.C0:].contiguous()
    outs = [ops.upconv_partial(s.gx1, a, d, pk, s.Cout, act_inv=inv).cpu().double() for pk in _both_packs(w, w.to(DEV).contiguous(), s.Cout, F16X2)]
    return s, outs, R.partial_reference(s.x1, at.cpu(), dt.cpu(), w1), _yardstick(s, w1, at, dt, F16X2)


def test_weight_row_outliers():
    """one output row x1000 and one single weight x1000: the error of every (class, row) relative to that (class, row)'s own largest value -- the pack
    keeps one power-of-two scale per (class, row) -- within max(2 * e32_rel, 2e-6) (test_conv3d_f16x2_small_activations_and_weight_outliers' bar)"""
    s = _setup(RAGGED_NARROW)
    w = s.w.clone()
    w[7] *= 1000.0
    w[3, R.C0 + 5, 0, 2, 1] *= 1000.0
    s, outs, ref, y32 = _rows_case(w)
    Cout = s.Cout
    scale = ref.abs().reshape(-1, 8 * Cout).amax(dim=0).clamp_min(1e-30)
    rel = lambda t: ((t - ref).abs().reshape(-1, 8 * Cout).amax(dim=0) / scale)   # noqa: E731
    e32 = float(rel(y32).max())
    assert float(scale.view(8, Cout)[:, 7].min()) > 100 * float(scale.view(8, Cout)[:, 8].max())      # the outlier row is one
    for name, out in zip(("host pack", "device pack"), outs):
        e16 = rel(out)
        print(f"[upconv-partial] weight outliers, {name}: per-(class, row) relative err {float(e16.max()):.2e} at (class, row) "
              f"{divmod(int(e16.argmax()), Cout)}, fp32-MFMA kernel {e32:.2e}")
        assert float(e16.max()) <= max(2 * e32, 2e-6), name
    assert torch.equal(outs[0], outs[1])


def test_weight_row_zero_and_cancelling_taps():
    """an all-zero output row: the partial is exactly 0.0 in all 8 classes of that row; a row with w[..., 0] == -w[..., 1] == w[..., 2] along x: the
    merged tap of two fine taps cancels to exactly 0 on the host for either parity -- both packs still meet bar (a)"""
    s = _setup(RAGGED_NARROW)
    w = s.w.clone()
    w[11] = 0.0
    w[13, :, :, :, 0] = -w[13, :, :, :, 1]
    w[13, :, :, :, 2] = -w[13, :, :, :, 1]
    wm = ops.polyphase_weights(w, R.C0)[1]
    assert bool((wm.view(8, s.Cout, s.C1, 3, 3, 3)[:, 13, :, :, :, 1] == 0).all()) and bool((wm.view(8, s.Cout, s.C1, 3, 3, 3)[:, 13] != 0).any())
    s, outs, ref, y32 = _rows_case(w)
    bar = 2 * max(float((y32 - ref).abs().max()), 2e-6)
    for name, out in zip(("host pack", "device pack"), outs):
        errs = R.class_errors(out, ref, s.Cout)
        print(f"[upconv-partial] zero row and cancelling taps, {name}: class errors [{', '.join(f'{e:.2e}' for e in errs)}], bar {bar:.2e}")
        assert max(errs) <= bar, name
        assert bool((out.reshape(-1, 8, s.Cout)[:, :, 11] == 0.0).all()), name
        assert float(out.reshape(-1, 8, s.Cout)[:, :, 13].abs().max()) > 0.1
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------- refusals
def test_entry_refusals_write_nothing():
    """gn_upconv_partial refuses by message, before any launch: the guarded buffer is unchanged, inside and out"""
    case = R.CASES[0]
    s = _setup(case)
    (Dc, Hc, Wc), C1, Cout, B = case
    host, _ = _packs(case, F16X2)
    buf = _guarded(B * Dc * Hc * Wc, 8 * Cout, inside=GUARD)
    good = dict(src1=s.gx1, C1=C1, a=s.a0, d=s.d0, wp=host.tensor, mode=F16X2, out_scale=host.out_scale, act_inv=None, B=B, Dc=Dc, Hc=Hc, Wc=Wc, Cout=Cout,
                partial=buf[PAD:])
    refusals = [(dict(mode=BF16X3), "two-plane modes only"), (dict(mode=0), "two-plane modes only"),
                (dict(C1=24), "channels must be multiples of 16"), (dict(C1=400), "channels must be multiples of 16"),
                (dict(Cout=48), "channels must be multiples of 16")]
    refusals += [(dict([(k, v)]), "bad sizes") for k, v in (("Dc", 0), ("Hc", -1), ("Wc", 0), ("B", -1), ("C1", 0), ("C1", -16), ("Cout", 0))]
    refusals += [(dict([(k, None)]), "null pointer") for k in ("src1", "a", "d", "wp", "out_scale", "partial")]
    for over, msg in refusals:
        with pytest.raises(ValueError, match="gn_upconv_partial: .*" + msg):
            _entry(**dict(good, **over))
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())
    # B = 0: nothing to do, whatever the pointers
    assert _entry(**dict(good, B=0, src1=None, partial=None)) == _lib.GN_OK
    empty = ops.upconv_partial(s.gx1[:0], s.a0[:0], s.d0[:0], host, Cout)
    assert empty.shape == (0, Dc, Hc, Wc, 8 * Cout)
    assert bool((buf == GUARD).all())
    # and the good arguments do launch
    _entry(**good)
    assert not bool((buf[PAD:PAD + B * Dc * Hc * Wc] == GUARD).any()) and _guards_untouched(buf, B * Dc * Hc * Wc)


def test_wrapper_refusals_before_any_launch(monkeypatch):
    """ops.upconv_partial raises TypeError / ValueError by name before any launch: the kernel reads src1, a1, d1, act_inv and the pack by the strides
    their documented shapes imply, so anything else would be silently wrong numbers"""
    case = RAGGED_NARROW
    s = _setup(case)
    C1, Cout, B = s.C1, s.Cout, s.B
    a, d, inv, _, _ = _affine(s, True)
    host, _ = _packs(case, F16X2)
    other, _ = _packs(R.CASES[0], F16X2)                                              # the pack of 16 -> 32
    want = ops.upconv_partial(s.gx1, a, d, host, Cout, act_inv=inv)

    def no_launch(name, *args):
        raise AssertionError(f"{name} launched")
    monkeypatch.setattr(_lib, "call", no_launch)
    full_a = torch.cat((torch.ones(B, R.C0, device=DEV), a), dim=1)                    # the layer's full-width rows [B][C0 + C1]
    SP = ops.SplitPack
    good = dict(src1=s.gx1, a1=a, d1=d, pack=host, cout=Cout, act_inv=inv)
    refusals = [
        (dict(src1=s.gx1.double()), TypeError, "src1"),
        (dict(src1=s.gx1.half()), TypeError, "src1"),
        (dict(src1=s.gx1.transpose(2, 3)), ValueError, "src1.*contiguous"),
        (dict(src1=s.gx1[..., ::2]), ValueError, "src1.*contiguous"),
        (dict(src1=s.gx1[0]), ValueError, "src1: expected"),
        (dict(src1=s.gx1.reshape(B, -1, C1)), ValueError, "src1: expected"),
        (dict(a1=full_a), ValueError, "a: expected"),
        (dict(d1=full_a), ValueError, "d: expected"),
        (dict(a1=full_a[:, R.C0:]), ValueError, "a.*contiguous"),
        (dict(a1=a[:1]), ValueError, "a: expected"),
        (dict(d1=d.reshape(-1)), ValueError, "d: expected"),
        (dict(a1=a.double()), TypeError, "a"),
        (dict(act_inv=inv[:, None]), ValueError, "act_inv: expected"),
        (dict(act_inv=inv[:1]), ValueError, "act_inv: expected"),
        (dict(act_inv=inv.double()), TypeError, "act_inv"),
        (dict(pack=other), ValueError, "pack: "),
        (dict(pack=SP(host.tensor[:-8], host.mode, host.out_scale)), ValueError, "pack: "),
        (dict(pack=SP(host.tensor, host.mode, host.out_scale[:Cout])), ValueError, "pack.out_scale: expected"),
        (dict(pack=SP(host.tensor, host.mode, host.out_scale.view(8, Cout))), ValueError, "pack.out_scale: expected"),
        (dict(pack=SP(host.tensor, BF16X3, host.out_scale)), ValueError, "two-plane modes only"),
    ]
    for over, exc, msg in refusals:
        with pytest.raises(exc, match=msg):
            ops.upconv_partial(**dict(good, **over))
    monkeypatch.undo()
    assert torch.equal(ops.upconv_partial(**good), want)                               # the conforming call is untouched
