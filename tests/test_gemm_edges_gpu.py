"""The split-precision GEMMs of mma_amd/csrc/gemm_x3.hip at their tile and dispatch boundaries: the smallest shapes at which a launch
ladder, a loop or a plan changes, against the float64 restatements of tests/gemm_ref.py under per-element bars, with NaN-padded pitched
operands, sentinel-guarded fp32 outputs (8 rows above, 32 below, columns on both sides) and the same bits on a second call.

  case                                                   kernel instantiation (entry point)
  test_a_every_accumulator_count        K = 128          gemm_x3_kernel<0, FULL, ACC>            (mma_gemm_bf16x3)
                                        K > 128, N/32    gemm_x3_kernel<1..4, FULL, ACC>; M < 128: FULL = false only, M = 128: FULL = true
                                                         only, M = 129 / 257: both
  test_a_grid_stride                                     gemm_x3_kernel<1, true, false> and <0, true, true> past 512 workgroups
  test_a_column_groups                  N = 384/640/4096 gemm_x3_colgroup_kernel with 3 / 5 / 32 groups (idle slots at 3 and 5) + the plain kernel
  test_a_n128_long_k                                     gemm_x3_n128_kernel<false / true> (+ gemm_x3_kernel<4, false, ACC> for the 255 rows left)
  test_a_column_blocks                                   bf16x3_blocks of dense: three launches of gemm_x3_kernel<4> into one pitched out
  test_b_rows_forms                     n128             gemm_f16x2_n128_kernel<0 / 2>           (mma_gemm_f16x2_n128)
                                        nlp              gemm_f16x2_nlp_kernel<4 / 8, 0 / 2>, n_kc = 4, 6, 8, 16  (mma_gemm_f16x2_nlp)
  test_b_grid_stride                                     both, a second unit per workgroup (M = 65 536 + 257)
  test_b_wide_rows                                       both, rows with a range of 2^30 inside
  test_c_row_independence                                every NN form + gemm_f16x2_colgroup_kernel<G2, KS> (mma_gemm_f16x2_k, K = 64 / 96 / 128)
  test_d_*                                               gemm_x3_tn_kernel<true / false>          (mma_gemm_bf16x3_tn), 1 .. 512 splits, an empty one
  test_e_*                                               gemm_f16x2_tn_kernel<FULL, 4 / 8, PACKED> (mma_gemm_f16x2_tn), the ragged eight-wave
                                                         kernel <false, 8, ..> at KA = 129 / 200 / 255, the device-side fall-back
  test_f_*                                               gemm_x3_tn_kernel, batched               (mma_gemm_bf16x3_tn_batched), an empty split
  test_g_*                                               split3_kernel, row_absmax (scalar / vector), pack_f16x2_k256_kernel +
                                                         gemm_f16x2_colgroup_k256_kernel<PACKED, CT> (mma_gemm_f16x2_k256 / _k256p and the `_h` twins)
The last tests of the file assert the yardstick of every form over its pooled cases and that every extern "C" entry point of gemm_x3.hip
was reached by the cases above (they need the whole file to have run).  524 cases, 12 s on an MI355X; the slowest takes 0.4 s."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import C_X, DEV

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mma_amd", "csrc", "gemm_x3.hip")
NO_SPREAD = ("big", "zero", "tiny")       # the last row a lone 1e36: rows whose range stays inside 2^16 (or that have one element)


@pytest.fixture
def rec(monkeypatch):
    return R.Recorder(monkeypatch)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_nn(what, rec, a, w, call, entry, c0=None, form=None, bar=None, kinds=R.EDGE_KINDS):
    """call(out) writes (or adds) a @ w into the guarded out: float64 bar, guards, no NaN from a pad, the entry point, the same bits again.
    The bar: C_X per element; an element of the rows that edge_matrix spread over e^+-20 inside (kinds) may exceed it and is then held
    to torch fp32 on the same rows (gemm_ref.assert_bar, dominated); bar(mag) where the case is about a bound."""
    M, N = a.shape[0], w.shape[1]
    spread = torch.zeros(M, device=DEV, dtype=torch.float64)
    spread[R.rows_of_kind(M, kinds, "spread")] = 1.0
    buf, out = R.guarded(M, N, fill=c0)
    rec.clear()
    call(out)
    got = out.clone()
    R.assert_guards_intact(buf, M, N, what)
    rec.assert_only(*entry)
    ref, mag = R.nn64(a, w, c0)
    if bar is not None:
        R.assert_bar(what, got, ref, mag, bar=bar(mag), c0=c0)
    else:
        own = mag - (c0.double().abs() if c0 is not None else 0)
        R.assert_bar(what, got, ref, mag, c0=c0, dominated=own * spread[:, None], f32=lambda: R.nn32(a, w, c0))
    if form:
        R.note_yardstick(form, got, R.nn32(a, w, c0), ref, mag)
    buf2, out2 = R.guarded(M, N, fill=c0)
    call(out2)
    assert same_bits(out2, got), "%s: a second call gives other bits" % what
    R.assert_guards_intact(buf2, M, N, what + " (second call)")
    return got


@functools.lru_cache(maxsize=8)
def nn_case(M, K, N, kinds=R.EDGE_KINDS):
    rng = rng_of("nn", M, K, N)
    a = R.pad_a(R.edge_matrix(M, K, rng, kinds=kinds))
    w = R.weights(K, N, rng)
    c0 = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).to(DEV)
    return a, w, c0


def split_bt3(w):
    """(3, N, K) bf16 pieces of w^T, as dense._run_bf16x3 makes them."""
    from mma_amd import dense
    K, N = w.shape
    wt = w.t().contiguous()
    bt3 = torch.empty((3, N, K), device=DEV, dtype=torch.bfloat16)
    dense.call("mma_split_bf16x3", wt, N * K, bt3, None)
    return bt3


# ---- a. six-product NN --------------------------------------------------------------------------------------------------------------------
NCT_CASES = [(128, 32), (128, 96), (128, 160)] + [(K, N) for K in (256, 384) for N in (32, 64, 96, 128)]


@pytest.mark.parametrize("M", [1, 31, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("K,N", NCT_CASES)
def test_a_every_accumulator_count(K, N, M, rec, monkeypatch):
    """gemm_x3_kernel<NCT, FULL, ACC>: tail only (M < 128), exactly one full block and no tail launch (128), a full block and a one-row
    tail (129, 257); accumulate=1 equals c0 + plain bit for bit."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    a, w, c0 = nn_case(M, K, N)
    what = "bf16x3 M=%d K=%d N=%d" % (M, K, N)
    plain = run_nn(what, rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out), ("mma_gemm_bf16x3",))
    acc = run_nn(what + " acc", rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out, accumulate=True), ("mma_gemm_bf16x3",), c0=c0)
    assert same_bits(acc, c0 + plain), what + ": accumulate is not c0 + plain"


@pytest.mark.parametrize("K,N", [(128, 160), (256, 64)])
def test_a_no_rows_no_launch(K, N, rec, monkeypatch):
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    a, w, _ = nn_case(33, K, N)
    buf, out = R.guarded(4, N, fill=7.0)
    keep = buf.clone()
    for acc in (0, 1):
        rec.call("mma_gemm_bf16x3", a, a.stride(0), split_bt3(w), out, out.stride(0), 0, N, K, acc, None)
        assert dense.gemm_bf16x3(a[:0], w, out=out[:0], accumulate=bool(acc)).shape == (0, N)
    assert same_bits(buf, keep)


@pytest.mark.parametrize("M,K,N,acc", [(65536 + 128 + 5, 256, 32, False), (65669, 128, 160, True)])
def test_a_grid_stride(M, K, N, acc, rec, monkeypatch):
    """More than 512 full blocks of 128 rows: a workgroup takes a second block (NCT = 1; NCT = 0 with ACC), then a 5-row tail."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    assert M // 128 > R.GRID_X3 and M % 128 == 5 and not (K == 128 and N % 128 == 0)
    a, w, c0 = nn_case(M, K, N)
    got = run_nn("bf16x3 grid-stride M=%d K=%d N=%d" % (M, K, N), rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out, accumulate=acc),
                 ("mma_gemm_bf16x3",), c0=c0 if acc else None, form="bf16x3")
    if acc:
        assert same_bits(got, c0 + dense.gemm_bf16x3(a, w))


@pytest.mark.parametrize("N", [384, 640, 4096])
def test_a_column_groups(N, rec, monkeypatch):
    """gemm_x3_colgroup_kernel with 3, 5 and 32 column groups (3 and 5 do not divide the 32 slots of an XCD: idle slots).  One call just
    below its admission (all of it on gemm_x3_kernel<0>), one at threshold + 3 * 256 + 128 + 5: units that do not divide the streams, one
    full 128-row block, a ragged tail.  "Same product order as gemm_x3_kernel: bitwise the same C": the rows of the large call equal the
    same rows from calls below the threshold."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    thr = R.colgroup_min_rows(N)
    assert thr == {384: 81920, 640: 49152, 4096: 8192}[N]
    M = thr + 3 * 256 + 128 + 5
    a, w, _ = nn_case(M, 128, N)
    big = run_nn("bf16x3 column groups M=%d N=%d" % (M, N), rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out), ("mma_gemm_bf16x3",),
                 form="bf16x3")
    lo = a[:thr - 1]
    low = run_nn("bf16x3 below the column groups M=%d N=%d" % (thr - 1, N), rec, lo, w, lambda out: dense.gemm_bf16x3(lo, w, out=out),
                 ("mma_gemm_bf16x3",))
    rest = dense.gemm_bf16x3(a[thr - 1:], w)
    assert same_bits(big[:thr - 1], low) and same_bits(big[thr - 1:], rest)


@pytest.mark.parametrize("K", [256, 192 + 64 * 3])
@pytest.mark.parametrize("M", [65536, 65536 + 255])
def test_a_n128_long_k(M, K, rec, monkeypatch):
    """gemm_x3_n128_kernel: N = 128, K > 128 from 256 units of 256 rows on; exactly 256 units and no tail, and one full block + 127 ragged
    rows behind them.  accumulate=1 (the L2 atomic add) equals c0 + plain bit for bit."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    assert M >= R.X3_N128_MIN_ROWS and K % 128 == 0
    a, w, c0 = nn_case(M, K, 128)
    what = "bf16x3 N=128 long K M=%d K=%d" % (M, K)
    plain = run_nn(what, rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out), ("mma_gemm_bf16x3",), form="bf16x3")
    acc = run_nn(what + " acc", rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out, accumulate=True), ("mma_gemm_bf16x3",), c0=c0, form="bf16x3")
    assert same_bits(acc, c0 + plain)


def test_a_column_blocks(rec, monkeypatch):
    """K > 128 and N > 128: one launch per 128-column block of a pitched out, and each writes its own block only."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    M, K, N = 4099, 256, 384
    assert dense.nn_form(M, K, N, named=True) == "bf16x3_blocks"
    a, w, c0 = nn_case(M, K, N)
    got = run_nn("bf16x3_blocks", rec, a, w, lambda out: dense.gemm_bf16x3(a, w, out=out), ("mma_gemm_bf16x3",), form="bf16x3")
    assert rec.names.count("mma_gemm_bf16x3") == 2 * 3          # both calls of run_nn: three launches each
    buf, out = R.guarded(M, N, fill=c0)
    rec.call("mma_gemm_bf16x3", a, a.stride(0), split_bt3(w[:, 128:256]), out[:, 128:256], out.stride(0), M, 128, K, 0, None)
    assert same_bits(out[:, 128:256], got[:, 128:256]) and same_bits(out[:, :128], c0[:, :128]) and same_bits(out[:, 256:], c0[:, 256:])
    R.assert_guards_intact(buf, M, N)


# ---- b. three-product NN with row maxima from outside ------------------------------------------------------------------------------------------
def raw_rows(rec, form, a, rm, w, out, acc):
    """mma_gemm_f16x2_nlp in one launch, or mma_gemm_f16x2_n128 once per 128-column block of out, through _lib.call."""
    from mma_amd import dense
    (M, K), N = a.shape, w.shape[1]
    bt2, cu = dense._split_f16x2(w, plain_lo=form == "nlp")
    if form == "nlp":
        rec.call("mma_gemm_f16x2_nlp", a, a.stride(0), rm, bt2, cu, out, out.stride(0), M, N, K, int(acc), None)
        return
    for b in range(N // 128):
        blk = bt2[:, 128 * b:128 * b + 128].contiguous()
        rec.call("mma_gemm_f16x2_n128", a, a.stride(0), rm, blk, cu[128 * b:], out[:, 128 * b:], out.stride(0), M, K, int(acc), None)


ROWS_CASES = [("n128", K, N) for K in (64, 192, 320) for N in (128, 384)] + [("nlp", K, N) for K in (256, 384, 512, 1024) for N in (128, 256)]


@pytest.mark.parametrize("M", [1, 31, 33, 255, 256, 257, 300])
@pytest.mark.parametrize("form,K,N", ROWS_CASES)
def test_b_rows_forms(form, K, N, M, rec):
    """mma_gemm_f16x2_n128 / _nlp below and around one 256-row unit (257: seven of eight wavefronts have no row but stage and meet the
    barriers), through dense.gemm_f16x2_n128 and through _lib.call (the same bits), row maxima exact / 8x loose / 0 on zero rows, both
    accumulate values; nlp at n_kc = 4 (the pipelined loop body never runs), 6 (once), 8 and 16.  Accumulating: the rows of all-zero A rows
    keep c0 bit for bit."""
    from mma_amd import dense
    assert dense._rows_form(K, N) == "f16x2_" + form
    entry = ("mma_gemm_f16x2_" + form,)
    kinds = R.EDGE_KINDS if form == "n128" else NO_SPREAD          # nlp's wide rows have their own case and bar (test_b_wide_rows)
    a, w, c0 = nn_case(M, K, N, kinds)
    rm = R.mixed_row_max(a)
    zero_rows = rm == 0
    assert bool(zero_rows.any()) or M < 2
    for acc in (False, True):
        what = "%s M=%d K=%d N=%d acc=%d" % (form, M, K, N, acc)
        c = c0 if acc else None
        got = run_nn(what, rec, a, w, lambda out: dense.gemm_f16x2_n128(a, rm, w, out, accumulate=acc), entry, c0=c, kinds=kinds)
        raw = run_nn(what + " raw", rec, a, w, lambda out: raw_rows(rec, form, a, rm, w, out, acc), entry, c0=c, kinds=kinds)
        assert same_bits(got, raw)
        if acc:
            assert same_bits(got[zero_rows], c0[zero_rows]), what + ": rows of all-zero A rows do not keep c0"


@pytest.mark.parametrize("form,N", [("n128", 128), ("nlp", 128), ("nlp", 256)])
def test_b_grid_stride(form, N, rec):
    """M = 65 536 + 257: the smallest M with more than 256 units - a workgroup runs a second unit (LDS buffer 0 is reused behind the
    prologue barrier) - whose last unit has one row."""
    M, K = 65536 + 257, 256
    assert -(-M // R.CG_ROWS) == R.GRID_UNITS + 2
    kinds = R.EDGE_KINDS if form == "n128" else NO_SPREAD
    a, w, c0 = nn_case(M, K, N, kinds)
    rm = R.mixed_row_max(a)
    for acc in (False, True):
        run_nn("%s grid-stride N=%d acc=%d" % (form, N, acc), rec, a, w, lambda out: raw_rows(rec, form, a, rm, w, out, acc),
               ("mma_gemm_f16x2_" + form,), c0=c0 if acc else None, form="f16x2_" + form, kinds=kinds)


@pytest.mark.parametrize("form,K,N", [("nlp", 256, 128), ("nlp", 512, 256), ("n128", 320, 128)])
@pytest.mark.parametrize("loose", [False, True])
def test_b_wide_rows(form, K, N, loose, rec):
    """A wide range INSIDE rows: row 5 has elements down to 2^-30 of its maximum; row 7 has large elements that meet tiny weights (2^-20)
    and small ones (2^-20) that meet ordinary weights, so that mag is not dominated by the large ones.  nlp: the header's bound,
    evaluated per element with the row maxima as passed (8x loose: three binades more of absolute error); n128 (two accumulators,
    lo pre-scaled by 2^11): C_X."""
    M = 33
    rng = rng_of("wide", form, K, N)
    a = R.edge_matrix(M, K, rng, kinds=NO_SPREAD)
    a[5] = torch.from_numpy((rng.standard_normal(K) * np.exp2(-rng.uniform(0, 30, K))).astype(np.float32))
    a[5, 3] = 1.5
    a[7] = torch.from_numpy(rng.standard_normal(K).astype(np.float32))
    a[7, K // 2:] *= 2.0 ** -20
    a = R.pad_a(a)
    w = R.weights(K, N, rng, col_spread=0.0)
    w[:K // 2] *= 2.0 ** -20
    rm = a.abs().amax(1) * (8.0 if loose else 1.0)

    def bar(mag):       # nlp: W's columns have a range of 2^20 inside as well, so the header's bound is the bar of every row here
        return R.nlp_header_bound(a, w, rm, mag) if form == "nlp" else C_X * mag
    c0 = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).to(DEV) * 2.0 ** -24
    for acc in (False, True):
        run_nn("%s wide rows K=%d N=%d loose=%d acc=%d" % (form, K, N, loose, acc), rec, a, w, lambda out: raw_rows(rec, form, a, rm, w, out, acc),
               ("mma_gemm_f16x2_" + form,), c0=c0 if acc else None, bar=bar)


# ---- c. row independence of every NN form ----------------------------------------------------------------------------------------------------
INDEP = [("bf16x3", 128, 160, 300), ("bf16x3", 256, 64, 300), ("bf16x3", 384, 128, 300), ("n128", 192, 128, 300), ("nlp", 256, 128, 300),
         ("nlp", 384, 256, 300), ("f16x2_k", 64, 256, 300), ("f16x2_k", 96, 384, 300), ("f16x2_k", 128, 256, 300), ("k256", 256, 256, 300),
         ("bf16x3", 256, 128, 65536 + 255), ("bf16x3", 128, 640, 49152 + 901)]


@pytest.mark.parametrize("form,K,N,M", INDEP, ids=["%s-K%d-N%d-M%d" % c for c in INDEP])
def test_c_row_independence(form, K, N, M, rec, monkeypatch):
    """Row i of C is a function of row i of A, of W and of row_max[i] alone: the first m rows of an M-row call equal an m-row call, and a
    row permutation of A permutes the rows of C - bit for bit (a wrong __shfl lane, a wrong clamp or a stale base row has no tolerance to
    hide in).  The two tall cases cross the 8-wave kernels' admission: their short calls run on gemm_x3_kernel."""
    from mma_amd import dense
    monkeypatch.setattr(dense, "USE_F16X2", False)
    a, w, _ = nn_case(M, K, N, NO_SPREAD)
    rm = R.mixed_row_max(a) if form in ("n128", "nlp") else a.abs().amax(1).contiguous()

    def run(a_, rm_):
        out = torch.full((a_.shape[0], N), float("nan"), device=DEV)
        if form == "bf16x3":
            dense.gemm_bf16x3(a_, w, out=out)
        elif form == "f16x2_k":
            dense.gemm_f16x2(a_, w, out=out)
        elif form == "k256":
            bt2, cu = dense._split_f16x2(w)
            rec.call("mma_gemm_f16x2_k256", a_, a_.stride(0), rm_, bt2, cu, out, N, a_.shape[0], N, None)
        else:
            raw_rows(rec, form, a_, rm_, w, out, False)
        return out
    full = run(a, rm)
    assert bool(torch.isfinite(full).all())
    rec.assert_only({"bf16x3": "mma_gemm_bf16x3", "f16x2_k": "mma_gemm_f16x2_k", "k256": "mma_gemm_f16x2_k256"}.get(form, "mma_gemm_f16x2_" + form))
    for m in (1, 33, 256):
        assert same_bits(run(a[:m], rm[:m].contiguous()), full[:m]), "the first %d rows of the %d-row call differ from a %d-row call" % (m, M, m)
    perm = torch.from_numpy(rng_of("perm", M).permutation(M)).to(DEV)
    assert same_bits(run(R.pad_a(a[perm]), rm[perm].contiguous()), full[perm]), "a row permutation of A does not permute the rows of C"


# ---- d. / e. TN ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def tn_case(M, KA, NC, three):
    """Six-product: X with every edge row (a lone 1e36 among them), G at 1e-3 with a lone 1e30 on a zero row of X and its lone 1e-30 on X's
    1e36, wide ranges inside the last row of both.  Three-product: ReLU rows spread over e^+-3 in both operands (2^17 in the row products, as
    in tests/test_gemm_gpu.py), G at 1e-3.
    Both: zero rows every 11th of X (from row 5) and every 13th of G (from row 7)."""
    rng = rng_of("tn", M, KA, NC, three)
    if three:
        xf = np.maximum(rng.standard_normal((M, KA)), 0) * np.exp(rng.uniform(-3, 3, (M, 1)))
        gf = rng.standard_normal((M, NC)) * 1e-3 * np.exp(rng.uniform(-3, 3, (M, 1)))
        xf, gf = torch.from_numpy(xf.astype(np.float32)), torch.from_numpy(gf.astype(np.float32))
    else:
        xf = R.edge_matrix(M, KA, rng, relu=True, kinds=X_KINDS)
        gf = R.edge_matrix(M, NC, rng, kinds=G_KINDS, big=1.0e30, scale=1e-3)
    xf[5::11] = 0
    gf[7::13] = 0
    return R.pad_x(xf), R.pad_x(gf)


def raw_tn(rec, form, x, g, xm=None, gm=None):
    """One call of mma_gemm_<form> through _lib.call: C (KA, NC) contiguous between guard rows, the workspace the size the library asks for,
    NaN-filled (a partial tile the kernel does not write shows) between guard rows of its own."""
    (M, KA), NC = x.shape, g.shape[1]
    n_ws = rec.query("mma_gemm_%s_workspace_floats" % form, M, KA, NC)
    bufw, ws = R.guarded_vec(n_ws) if n_ws else (None, None)
    bufc, C = R.guarded_flat(KA, NC)
    maxima = (xm, gm) if form == "f16x2_tn" else ()
    rec.call("mma_gemm_" + form, x, x.stride(0), g, g.stride(0), *maxima, C, ws, n_ws, M, KA, NC, None)
    got = C.clone()
    R.assert_flat_guards_intact(bufc, KA, "C")
    if bufw is not None:
        R.assert_vec_guards_intact(bufw, n_ws, "workspace")
    return got


X_KINDS, G_KINDS = ("spread", "zero", "big", "tiny"), ("spread", "big", "tiny", "zero")      # a 1e36 of X meets a 1e-30 of G, never a 1e30


def tn_dominated(x, g):
    """The part of mag that the rows spread inside in X and G contribute (and the lone 1e36 of X, one term that is all of its element): known
    from the population.  Where it is more than half of mag an element may exceed C_X and is held to torch fp32 (gemm_ref.assert_bar)."""
    M = x.shape[0]
    e = R.rows_of_kind(M, X_KINDS, "spread") + R.rows_of_kind(M, X_KINDS, "big")
    return x[e].double().abs().t() @ g[e].double().abs()


def run_tn(what, rec, form, x, g, xm=None, gm=None, bar=None, pool=None):
    """bar(mag) where the case is about a bound; else six-product: C_X, the dominated elements against torch fp32; three-product:
    gemm_ref.three_product_bar."""
    got = raw_tn(rec, form, x, g, xm, gm)
    ref, mag = R.tn64(x, g)
    M, KA, NC = x.shape[0], x.shape[1], g.shape[1]
    if bar is None and form == "bf16x3_tn":
        R.assert_bar(what, got, ref, mag, dominated=tn_dominated(x, g), f32=lambda: x.t().contiguous() @ g.contiguous())
    else:
        R.assert_bar(what, got, ref, mag, bar=bar(mag) if bar else R.three_product_bar(x, g, mag))
    if pool:
        R.note_yardstick(pool, got, x.t().contiguous() @ g.contiguous(), ref, mag)
    assert same_bits(raw_tn(rec, form, x, g, xm, gm), got), "%s: a second call gives other bits" % what
    return got


TN_SHAPES = [(1, 1), (8, 31), (31, 33), (32, 32), (33, 127), (100, 128), (128, 129), (128, 300), (32, 128), (1, 300)]


@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 65, 128, 129, 1000])
@pytest.mark.parametrize("KA,NC", TN_SHAPES)
def test_d_six_product_tn(KA, NC, M, rec):
    """mma_gemm_bf16x3_tn from one row on: one chunk, one ragged chunk, 1 .. 3 splits, ragged and whole tiles (gemm_x3_tn_kernel<false> and
    <true> at (32, 128)), NaN-padded pitched X and G."""
    x, g = tn_case(M, KA, NC, False)
    run_tn("bf16x3_tn M=%d KA=%d NC=%d" % (M, KA, NC), rec, "bf16x3_tn", x, g)


def test_d_an_empty_split_writes_zeros(rec):
    """(128, 32, 32) is planned as 3 splits of 64 rows: the third starts at row 128 and has none; its partial tile must still be written (as
    zeros) before mma_col_sum adds it - the workspace starts as NaN.  One more row gives that split one row."""
    assert R.tn_splits(128, 32, 32) == 3 and R.tn_rows_per_split(128, 3) == 64 and 2 * 64 >= 128
    assert R.tn_splits(129, 32, 32) == 3 and 2 * R.tn_rows_per_split(129, 3) == 128
    for M in (128, 129):
        x, g = tn_case(M, 32, 32, False)
        run_tn("bf16x3_tn empty split M=%d" % M, rec, "bf16x3_tn", x, g)


@pytest.mark.parametrize("M", [65535, 65536])
def test_d_plan_change_at_65536_rows(M, rec):
    """2 chunks per split at least below 65 536 rows (512 splits of 128 rows), 8 from there on (256 splits of 256 rows)."""
    s = R.tn_splits(M, 32, 32)
    assert (s, R.tn_rows_per_split(M, s)) == ((512, 128) if M < 65536 else (256, 256))
    x, g = tn_case(M, 32, 32, False)
    run_tn("bf16x3_tn plan M=%d" % M, rec, "bf16x3_tn", x, g)


def test_d_yardstick_case(rec):
    x, g = tn_case(1000, 128, 640, False)
    run_tn("bf16x3_tn M=1000 KA=128 NC=640", rec, "bf16x3_tn", x, g, pool="bf16x3_tn")


@pytest.mark.parametrize("M", [129, 1000])
@pytest.mark.parametrize("KA,k,NC,n", [(100, 33, 300, 257), (128, 100, 128, 97), (33, 1, 129, 129)])
def test_d_bit_relations(KA, k, NC, n, M, rec):
    """Same M and the same number of 128-column blocks (so the same plan): the result for X[:, :k] is the first k rows of the result for X,
    the result for G[:, :n] its first n columns, and a column permutation of X permutes the rows of C - "columns past KA repeat the last
    one: they only reach rows that are never stored"."""
    assert -(-n // 128) == -(-NC // 128)
    x, g = tn_case(M, KA, NC, False)
    full = raw_tn(rec, "bf16x3_tn", x, g)
    assert same_bits(raw_tn(rec, "bf16x3_tn", x[:, :k], g), full[:k])
    assert same_bits(raw_tn(rec, "bf16x3_tn", R.pad_x(x[:, :k]), g), full[:k])              # ... with NaN right behind column k
    assert same_bits(raw_tn(rec, "bf16x3_tn", x, g[:, :n]), full[:, :n])
    assert same_bits(raw_tn(rec, "bf16x3_tn", x, R.pad_x(g[:, :n])), full[:, :n])
    perm = torch.from_numpy(rng_of("cols", KA).permutation(KA)).to(DEV)
    assert same_bits(raw_tn(rec, "bf16x3_tn", R.pad_x(x[:, perm]), g), full[perm])


def tn_maxima(x, g, mode):
    if mode == "own":
        return None, None
    xm, gm = x.abs().amax(1).contiguous(), g.abs().amax(1).contiguous()
    return (xm * 8.0, gm * 3.0) if mode == "loose" else (xm, gm)


@pytest.mark.parametrize("maxima", ["given", "loose", "own"])
@pytest.mark.parametrize("M", [1, 33, 128, 129, 1000, 65535, 65536])
@pytest.mark.parametrize("KA,NC", [(8, 31), (32, 32), (33, 127), (100, 128), (128, 300)])
def test_e_three_product_tn(KA, NC, M, maxima, rec):
    """mma_gemm_f16x2_tn at the shapes of d.: row maxima given, 8x / 3x loose, NULL (the kernel's own pass)."""
    x, g = tn_case(M, KA, NC, True)
    xm, gm = tn_maxima(x, g, maxima)
    got = run_tn("f16x2_tn M=%d KA=%d NC=%d %s" % (M, KA, NC, maxima), rec, "f16x2_tn", x, g, xm, gm)
    if M >= 1000:
        assert not same_bits(got, raw_tn(rec, "bf16x3_tn", x, g))           # the three-product kernel did the work, not the fall-back


@pytest.mark.parametrize("M", [33, 1000, 65536])
@pytest.mark.parametrize("KA,NC", [(33, 127), (100, 300), (128, 128), (200, 96)])
def test_e_packed_x_is_bit_equal(KA, NC, M, rec, monkeypatch):
    """MMA_TN_PACKX 0 and 1 (read per call; the workspace query grows with it): the same bits, on ragged KA as well."""
    x, g = tn_case(M, KA, NC, True)
    xm, gm = tn_maxima(x, g, "given")
    res = {}
    for v in ("0", "1"):
        monkeypatch.setenv("MMA_TN_PACKX", v)
        res[v] = run_tn("f16x2_tn packx=%s M=%d KA=%d NC=%d" % (v, M, KA, NC), rec, "f16x2_tn", x, g, xm, gm)
    assert same_bits(res["0"], res["1"])


@pytest.mark.parametrize("M", [33, 1000])
@pytest.mark.parametrize("NC", [96, 128, 300])
@pytest.mark.parametrize("KA", [129, 200, 255, 256])
def test_e_eight_wave_kernel(KA, NC, M, rec):
    """Through _lib.call the entry takes any KA <= 256 (dense only ever sends 256): gemm_f16x2_tn_kernel<false, 8, ..> on ragged KA.  It must
    equal, bit for bit, one call per 128-column block of X with the same row maxima - what the header promises for KA = 256."""
    x, g = tn_case(M, KA, NC, True)
    xm, gm = tn_maxima(x, g, "given")
    got = run_tn("f16x2_tn eight waves M=%d KA=%d NC=%d" % (M, KA, NC), rec, "f16x2_tn", x, g, xm, gm, pool="f16x2_tn")
    blocks = torch.cat([raw_tn(rec, "f16x2_tn", x[:, j:j + 128], g, xm, gm) for j in (0, 128)])
    assert same_bits(got, blocks)


@pytest.mark.parametrize("KA", [100, 200])
@pytest.mark.parametrize("case", ["spread", "inf", "nan", "subnormal", "zero"])
def test_e_device_side_fall_back_at_small_m(case, KA, rec):
    """A row 2^50 away, an inf / NaN / subnormal row maximum: the bits of the six-product kernel; all-zero X: exact zeros.  KA = 200 goes
    through dense (128 + 72 columns: two launches)."""
    from mma_amd import dense
    M, NC = 129, 96
    x, g = tn_case(M, KA, NC, True)
    x, g = x.clone(), g.clone()
    if case == "spread":
        x[5 + 1] *= 2.0 ** 50
    elif case == "inf":
        x[40, 5::128] = float("inf")
    elif case == "nan":
        g[41, 7] = float("nan")
    elif case == "subnormal":
        x[42] = 1e-41
        x[42, 3] = 3e-39
    else:
        x[:] = 0
    rec.clear()
    if KA > 128:
        got, six = dense.gemm_f16x2_tn(x, g), dense.gemm_bf16x3_tn(x, g)
        assert rec.names.count("mma_gemm_f16x2_tn") == 2 and rec.names.count("mma_gemm_bf16x3_tn") == 2
    else:
        got, six = raw_tn(rec, "f16x2_tn", x, g), raw_tn(rec, "bf16x3_tn", x, g)
    if case == "zero":
        assert same_bits(got, torch.zeros_like(got))
        return
    assert torch.equal(got.isnan(), six.isnan()) and same_bits(got.nan_to_num(0.0, 1.0, -1.0), six.nan_to_num(0.0, 1.0, -1.0))


@pytest.mark.parametrize("case", ["spread", "small rows"])
def test_e_header_bound(case, rec):
    """|error| <= 2^-22 sum|x||g| + M 2^-39 max_i(max|x_i| max|g_i|), per element, with the maxima as passed (8x / 3x loose).  spread: rows
    over 2^+-17 against each other; small rows: one large row and 4 095 rows whose products lie 2^-35 below it - the case of the second term."""
    M, KA, NC = 4096, 100, 300
    rng = rng_of("tn bound", case)
    xf = np.maximum(rng.standard_normal((M, KA)), 0)
    gf = rng.standard_normal((M, NC))
    if case == "spread":
        xf *= np.exp2(rng.uniform(-8.5, 8.5, (M, 1)))
        gf *= np.exp2(rng.uniform(-8.5, 8.5, (M, 1)))
    else:
        xf[1:] *= 2.0 ** -17
        gf[1:] *= 2.0 ** -18
    x, g = R.pad_x(torch.from_numpy(xf.astype(np.float32))), R.pad_x(torch.from_numpy(gf.astype(np.float32)))
    xm, gm = tn_maxima(x, g, "loose")
    got = run_tn("f16x2_tn header bound, " + case, rec, "f16x2_tn", x, g, xm, gm, bar=lambda mag: R.tn_header_bound(xm, gm, mag, M))
    assert not same_bits(got, raw_tn(rec, "bf16x3_tn", x, g))


# ---- f. batched TN ---------------------------------------------------------------------------------------------------------------------------
def towers(M, ka, nc, B, xgap, ggap, seed):
    """X (M, B * (ka + xgap) - xgap) and G likewise between NaN pads, gap columns NaN; the tower offsets."""
    rng = rng_of("towers", M, ka, nc, B, seed)
    xb, gb = ka + xgap, nc + ggap
    X = torch.full((M, xb * (B - 1) + ka), float("nan"))
    G = torch.full((M, gb * (B - 1) + nc), float("nan"))
    for b in range(B):
        X[:, b * xb:b * xb + ka] = R.edge_matrix(M, ka, rng, relu=True, kinds=X_KINDS)
        G[:, b * gb:b * gb + nc] = R.edge_matrix(M, nc, rng, kinds=G_KINDS, big=1.0e30, scale=1e-3)
    return R.pad_x(X), R.pad_x(G), xb, gb


def check_towers(what, got, X, G, ka, nc, B, xb, gb, pool=None):
    assert got.shape == (B, ka, nc)
    for b in range(B):
        x, g = X[:, b * xb:b * xb + ka], G[:, b * gb:b * gb + nc]
        ref, mag = R.tn64(x, g)
        R.assert_bar("%s tower %d" % (what, b), got[b], ref, mag, dominated=tn_dominated(x, g), f32=lambda: x.t().contiguous() @ g.contiguous())
        if pool:
            R.note_yardstick(pool, got[b], x.t().contiguous() @ g.contiguous(), ref, mag)


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("ka,nc", [(8, 32), (48, 152), (128, 129), (128, 640)])
def test_f_batched_tn(ka, nc, B, rec):
    """dense.xt_g_batched at M = 4 096 + 33: every tower against float64 per element (C_X; what the spread rows dominate against torch fp32); one
    row fewer than 4 096 and it falls back to one xt_g per tower, under the same bar."""
    from mma_amd import dense
    M = 4096 + 33
    X, G, xb, gb = towers(M, ka, nc, B, 0, 0, 0)
    rec.clear()
    got = dense.xt_g_batched(X, ka, G, nc, B)
    rec.assert_only("mma_gemm_bf16x3_tn_batched")
    check_towers("batched M=%d (%d, %d) B=%d" % (M, ka, nc, B), got, X, G, ka, nc, B, xb, gb, pool="bf16x3_tn_batched")
    assert same_bits(dense.xt_g_batched(X, ka, G, nc, B), got)
    if (ka, nc) == (48, 152):
        rec.clear()
        Ms = 4095
        got = dense.xt_g_batched(X[:Ms], ka, G[:Ms], nc, B)
        rec.assert_only("mma_gemm_bf16x3_tn")
        assert rec.names.count("mma_gemm_bf16x3_tn") == B
        check_towers("per tower M=%d (%d, %d) B=%d" % (Ms, ka, nc, B), got, X[:Ms], G[:Ms], ka, nc, B, xb, gb)


@pytest.mark.parametrize("ka,nc,B", [(48, 152, 5), (8, 32, 2), (33, 129, 3)])
def test_f_batched_tn_raw_with_gaps(ka, nc, B, rec):
    """Through _lib.call: towers with gaps (xb > ka, gb > nc) whose gap columns are NaN, a pitch with NaN pads, the output between guard
    rows, a NaN workspace.  (48, 152, B = 5) is planned as 16 splits of 288 rows: the last one is empty."""
    M = 4096 + 33
    s = R.tn_splits_batched(M, ka, nc, B)
    if (ka, nc, B) == (48, 152, 5):
        assert s == 16 and R.tn_rows_per_split(M, s) == 288 and 15 * 288 >= M
    X, G, xb, gb = towers(M, ka, nc, B, 3, 5, 1)
    n_ws = rec.query("mma_gemm_bf16x3_tn_batched_workspace_floats", M, ka, nc, B)
    assert n_ws == s * B * ka * nc

    def run():
        bufw, ws = R.guarded_vec(n_ws)
        bufc, C = R.guarded_flat(B * ka, nc)
        rec.call("mma_gemm_bf16x3_tn_batched", X, X.stride(0), xb, G, G.stride(0), gb, C, ws, n_ws, M, ka, nc, B, None)
        got = C.clone().view(B, ka, nc)
        R.assert_flat_guards_intact(bufc, B * ka, "C")
        R.assert_vec_guards_intact(bufw, n_ws, "workspace")
        return got
    got = run()
    check_towers("batched raw (%d, %d) B=%d" % (ka, nc, B), got, X, G, ka, nc, B, xb, gb)
    assert same_bits(run(), got)


# ---- g. the small helpers the forms depend on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_g_split_bf16x3(n, rec):
    """The three bf16 pieces sum back to the input exactly; the element behind the 3n written ones keeps a sentinel."""
    rng = rng_of("split", n)
    v = rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))
    v[0] = 1.0e36
    if n > 3:
        v[1], v[2], v[3] = 1.0e-30, 0.0, -3.0
    src = torch.from_numpy(v.astype(np.float32)).to(DEV)
    out = torch.full((3 * n + 1,), 0x7B7B, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    rec.call("mma_split_bf16x3", src, n, out, None)
    assert int(out.view(torch.int16)[3 * n]) == 0x7B7B
    pieces = out[:3 * n].view(3, n).double()
    assert torch.equal(pieces[0] + pieces[1] + pieces[2], src.double())


@pytest.mark.parametrize("M", [1, 7, 8, 9])
@pytest.mark.parametrize("cols,left,right", [(33, 1, 1), (75, 1, 2), (7, 3, 0), (64, 4, 4), (256, 0, 4), (4, 4, 0)])
def test_g_row_absmax(cols, left, right, M, rec):
    """mma_row_absmax: the scalar form (cols % 4 != 0, an odd pitch, a base that is 4-byte aligned only) and the vector form, NaN pads."""
    rng = rng_of("absmax", cols, M)
    a = R.nan_padded(R.edge_matrix(M, cols, rng), left, right)
    buf = torch.full((M + 2,), R.SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    rec.call("mma_row_absmax", a, a.stride(0), M, cols, buf[1:], None)
    assert same_bits(buf[1:1 + M], a.abs().amax(1)) and int(buf.view(torch.int32)[0]) == R.SENTINEL and int(buf.view(torch.int32)[M + 1]) == R.SENTINEL
    from mma_amd import dense
    assert same_bits(dense.row_absmax(a), a.abs().amax(1))


@pytest.mark.parametrize("M", [1, 31, 33, 257])
def test_g_k256_packed_equals_unpacked(M, rec):
    """mma_pack_f16x2_k256 + mma_gemm_f16x2_k256p against mma_gemm_f16x2_k256 bit for bit below the 65 536 rows dense asks for, and both
    against float64; the bf16 twins round those bits."""
    from mma_amd import dense
    N = 256
    a, w, _ = nn_case(M, 256, N)
    bt2, cu = dense._split_f16x2(w)
    rm = a.abs().amax(1).contiguous()
    n_bytes = rec.query("mma_pack_f16x2_k256_bytes", M)
    ap = torch.empty((n_bytes,), device=DEV, dtype=torch.uint8)
    sce = torch.empty((M,), device=DEV, dtype=torch.int32)
    rm_out = torch.empty((M,), device=DEV)
    rec.call("mma_pack_f16x2_k256", a, a.stride(0), M, ap, sce, rm_out, None)
    assert same_bits(rm_out, rm)
    plain = run_nn("f16x2_k256 M=%d" % M, rec, a, w, lambda out: rec.call("mma_gemm_f16x2_k256", a, a.stride(0), rm, bt2, cu, out, out.stride(0), M, N, None),
                   ("mma_gemm_f16x2_k256",))
    packed = run_nn("f16x2_k256p M=%d" % M, rec, a, w, lambda out: rec.call("mma_gemm_f16x2_k256p", ap, sce, bt2, cu, out, out.stride(0), M, N, None),
                    ("mma_gemm_f16x2_k256p",))
    assert same_bits(plain, packed)
    want = plain.to(torch.bfloat16).view(torch.int16)
    for name, args in (("mma_gemm_f16x2_k256_h", (a, a.stride(0), rm, bt2, cu)), ("mma_gemm_f16x2_k256p_h", (ap, sce, bt2, cu))):
        h = torch.zeros((M, N), device=DEV, dtype=torch.bfloat16)
        rec.call(name, *args, h, N, M, N, None)
        assert torch.equal(h.view(torch.int16), want), name


@pytest.mark.parametrize("M", [1, 33, 257])
@pytest.mark.parametrize("K,N", [(64, 384), (96, 256), (128, 128)])
def test_g_whole_row_form_by_every_name(K, N, M, rec):
    """mma_gemm_f16x2_k at K = 64 / 96 / 128 with three, two and one resident column groups on a ragged unit, guarded; K = 128 is
    mma_gemm_f16x2's product; the bf16 twin rounds the same bits."""
    from mma_amd import dense
    a, w, _ = nn_case(M, K, N)
    bt2, cu = dense._split_f16x2(w)
    got = run_nn("f16x2_k M=%d K=%d N=%d" % (M, K, N), rec, a, w, lambda out: dense.gemm_f16x2(a, w, out=out), ("mma_gemm_f16x2_k",))
    if K == 128:
        old = run_nn("f16x2 M=%d" % M, rec, a, w, lambda out: rec.call("mma_gemm_f16x2", a, a.stride(0), bt2, cu, out, out.stride(0), None, M, N, None),
                     ("mma_gemm_f16x2",))
        assert same_bits(old, got)
    h = torch.zeros((M, N), device=DEV, dtype=torch.bfloat16)
    rec.call("mma_gemm_f16x2_k_h", a, a.stride(0), bt2, cu, h, N, None, M, N, K, None)
    assert torch.equal(h.view(torch.int16), got.to(torch.bfloat16).view(torch.int16))


# ---- the yardstick and the coverage: after every case above ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16x3", "f16x2_n128", "f16x2_nlp", "bf16x3_tn", "f16x2_tn", "bf16x3_tn_batched"])
def test_z_yardstick(form):
    """Over the pooled cases of the form with at least 2^16 output elements: e_got <= 1.5 * e_f32 + 1e-7, torch fp32 on the same GPU."""
    R.assert_yardstick(form)


def test_z_every_entry_point_was_reached():
    missing = set(R.hip_entry_points(HIP)) - R.REACHED
    assert not missing, ("extern \"C\" entry points of gemm_x3.hip that no case which ran before this one in this process reached (run the "
                         "whole file, in file order): %r" % sorted(missing))
