"""K13 / K14 / K15 / K16 (mma_amd/csrc/tower_post.hip) at their plan and LDS limits, against float64 under per-element bars
(tests/tower_post_ref.py): more than one node tile per wavefront (the plan-sweep variables force at small N what the planner picks
above N ~ 8e4), K15 node ranges longer than 64 nodes and more than one kf pass, the col_sum fallback of the weight gradient, the
shapes next to the 160 KB LDS limit mma_tower_post_fits promises, rows of very different sizes, and - through the raw entry points -
row-strided buffers whose padding is NaN on the way in and a sentinel on the way out."""
import functools

import numpy as np
import pytest
import torch

import tower_post_ref as R
from tower_post_ref import C_GW, C_Y, SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AVG_LOG, AVG_LIN = 1.3, 2.2
SENT = -12345.75                                               # exactly representable: an untouched output element still holds it
PLAN_VARS = ("MMA_POST_TPW", "MMA_POST_TPW_ALL", "MMA_SKINNY_TPW", "MMA_POST_GW_WAVES", "MMA_POST_GW_TILES", "MMA_POST_EXACT", "MMA_POST_ORDER",
             "MMA_SKINNY_X3", "MMA_SKINNY_GW_WAVES")


@pytest.fixture(autouse=True)
def _no_plan_variables(monkeypatch):
    for v in PLAN_VARS:
        monkeypatch.delenv(v, raising=False)


def _setenv(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


# ---- cases: inputs and their float64 reference, computed once per shape and left unchanged ---------------------------------------
@functools.lru_cache(maxsize=None)
def _tower_case(N, T, KF, O, scalers, edges=False):
    rng = np.random.default_rng(1000 * N + 10 * KF + T + len(scalers))
    S = len(scalers)
    agg = torch.from_numpy(rng.standard_normal((N, T, KF)).astype(np.float32))
    Wo = torch.from_numpy((rng.standard_normal((T, O, S * KF)) / np.sqrt(S * KF)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((N, T * O)).astype(np.float32))
    if edges:
        deg = R.edge_degrees(N, rng)
        agg, cot = R.edge_rows(agg, rng, first=3), R.edge_rows(cot, rng, first=11)
    else:
        deg = torch.from_numpy(rng.integers(0, 7, N))
        deg[::17] = 0
    ref = R.tower_post64(agg, Wo, R.pre64(deg, scalers, AVG_LOG, AVG_LIN), cot)
    assert max(ref[k].max().item() for k in ("mag_y", "mag_ga", "mag_gw")) < 1e37, "the case itself leaves the fp32 range"
    return dict(N=N, T=T, KF=KF, O=O, S=S, scalers=scalers, deg=deg, rowptr=R.rowptr_of(deg).to(DEV), agg=agg.to(DEV), Wo=Wo.to(DEV),
                cot=cot.to(DEV), ref=ref)


def _tower_run(c, need_w=True):
    """Fn.tower_post forward + backward -> (y, gagg, gWo) on the CPU."""
    from mma_amd import functional as Fn
    ad, wd = c["agg"].clone().requires_grad_(True), c["Wo"].clone().requires_grad_(need_w)
    y = Fn.tower_post(ad, wd, c["rowptr"], list(c["scalers"]), AVG_LOG, AVG_LIN)
    gr = torch.autograd.grad((y * c["cot"]).sum(), [ad, wd] if need_w else [ad])
    torch.cuda.synchronize()
    return y.detach().cpu(), gr[0].cpu(), (gr[1].cpu() if need_w else None)


def _pre_table(c):
    """The fp32 scaler table the kernels read (mma_tower_post_pre), (N, S)."""
    from mma_amd._lib import call, host_codes, ptr, stream_ptr
    from mma_amd.functional import GR_SCALER
    pre = torch.zeros((c["N"], 8), device=DEV)
    call("mma_tower_post_pre", ptr(c["rowptr"]), ptr(pre), c["N"], c["S"], host_codes(GR_SCALER[s] for s in c["scalers"]), AVG_LOG, AVG_LIN, stream_ptr())
    return pre[:, :c["S"]].contiguous()


def _tower_bars(c, y, ga, gw, tag):
    ref, name = c["ref"], "%s %s" % ((c["N"], c["T"], c["KF"], c["O"], c["S"]), tag)
    R.assert_bar("y    " + name, y, ref["y"], ref["mag_y"], C_Y)
    if "ga32" not in c:
        c["ga32"] = R.tower_post32(c["agg"], c["Wo"], _pre_table(c), c["cot"]).cpu()
    R.assert_ga_bar("gagg " + name, ga, c["ga32"], ref["gagg"], ref["mag_ga"], c["S"])
    if gw is not None:
        R.assert_bar("gWo  " + name, gw, ref["gWo"], ref["mag_gw"], C_GW)


@functools.lru_cache(maxsize=None)
def _linear_case(N, K, O, edges=False):
    rng = np.random.default_rng(100 * N + 10 * K + O)
    x = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(O).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((N, O)).astype(np.float32))
    if edges:
        x, cot = R.edge_rows(x, rng, first=3), R.edge_rows(cot, rng, first=11)
    refs = {True: R.linear64(x, W, b, cot), False: R.linear64(x, W, None, cot)}
    assert max(refs[True][k].max().item() for k in ("mag_y", "mag_gx", "mag_gw")) < 1e37, "the case itself leaves the fp32 range"
    c = dict(N=N, K=K, O=O, x=x.to(DEV), W=W.to(DEV), b=b.to(DEV), cot=cot.to(DEV), refs=refs)
    c["gx32"] = (c["cot"] @ c["W"]).cpu()                       # the yardstick of c_ga: torch fp32 on the GPU
    return c


def _linear_run(c, bias):
    from mma_amd import dense
    xd, wd = c["x"].clone().requires_grad_(True), c["W"].clone().requires_grad_(True)
    bd = c["b"].clone().requires_grad_(True) if bias else None
    assert dense._skinny_ok(xd, wd), "this shape must take the K16 path"
    y = dense.linear(xd, wd, bd)
    gr = torch.autograd.grad((y * c["cot"]).sum(), [xd, wd] + ([bd] if bias else []))
    torch.cuda.synchronize()
    return (y.detach().cpu(),) + tuple(g.cpu() for g in gr)


def _linear_bars(c, bias, out, tag):
    ref, name = c["refs"][bias], "%s %s" % ((c["N"], c["K"], c["O"]), tag)
    R.assert_bar("y    " + name, out[0], ref["y"], ref["mag_y"], C_Y)
    R.assert_ga_bar("gx   " + name, out[1], c["gx32"], ref["gx"], ref["mag_gx"], -(-c["O"] // 16))
    R.assert_bar("gW   " + name, out[2], ref["gW"], ref["mag_gw"], C_GW)
    if bias:
        R.assert_bar("gb   " + name, out[3], ref["gb"], ref["mag_gb"], C_GW)


# ---- a. tiles per wavefront --------------------------------------------------------------------------------------------------------
TPW_SHAPES = [(321, 3, 36, 15, tuple(SC[:3])), (1153, 2, 100, 7, tuple(SC[1:3])), (1, 1, 4, 1, tuple(SC[:1]))]


@pytest.mark.parametrize("order", ["0", "2"])
@pytest.mark.parametrize("exact", [None, "1"], ids=["bf16x3_forward", "fp32_forward"])
@pytest.mark.parametrize("N,T,KF,O,scalers", TPW_SHAPES, ids=["6_tiles", "19_tiles", "1_node"])
def test_a_node_does_not_know_which_wave_walks_it(N, T, KF, O, scalers, exact, order, monkeypatch):
    """MMA_POST_TPW_ALL (MMA_SKINNY_TPW where T = 1: post_tiles_per_wave() reads one or the other) = 2, 3, 8 tiles per wavefront in K13
    and K14: the tile loop of the fp32 forward, the step walk of the bf16-piece forward, K14's two-set prefetch ring with odd tile counts,
    waves with no tile at all and a prefetch past N.  The arithmetic of a node is the same whichever wave walks it: y and gagg bit-equal
    to the one-tile plan, which is inside the bars.  MMA_POST_TPW moves the forward alone."""
    c = _tower_case(N, T, KF, O, scalers)
    _setenv(monkeypatch, MMA_POST_EXACT=exact, MMA_POST_ORDER=order, MMA_POST_TPW_ALL=1, MMA_SKINNY_TPW=1)
    y1, ga1, _ = _tower_run(c, need_w=False)
    _tower_bars(c, y1, ga1, None, "exact=%s order=%s" % (exact, order))
    for tpw in (2, 3, 8):
        _setenv(monkeypatch, MMA_POST_TPW_ALL=tpw, MMA_SKINNY_TPW=tpw)
        y, ga, _ = _tower_run(c, need_w=False)
        assert torch.equal(y, y1), ("y", tpw)
        assert torch.equal(ga, ga1), ("gagg", tpw)
    _setenv(monkeypatch, MMA_POST_TPW_ALL=None, MMA_SKINNY_TPW=None)
    for tpw in (1, 2, 3, 8):
        _setenv(monkeypatch, MMA_POST_TPW=tpw)
        y, ga, _ = _tower_run(c, need_w=False)
        assert torch.equal(y, y1) and torch.equal(ga, ga1), ("MMA_POST_TPW", tpw)


@pytest.mark.parametrize("x3", [None, "0"], ids=["bf16x3_forward", "fp32_forward"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("N,K,O", [(4097 + 64, 75, 75), (4200, 128, 16), (4161, 50, 80)])
def test_skinny_linear_does_not_depend_on_the_tiles_per_wave(N, K, O, bias, x3, monkeypatch):
    """K16 under MMA_SKINNY_TPW = 1, 2, 3, 8 (66 tiles: at 3 and 8 the last workgroup has waves with fewer tiles and with none): y and gx
    bit-equal to the one-tile plan, everything inside the bars."""
    c = _linear_case(N, K, O)
    _setenv(monkeypatch, MMA_SKINNY_X3=x3, MMA_SKINNY_TPW=1)
    base = _linear_run(c, bias)
    _linear_bars(c, bias, base, "bias=%s x3=%s" % (bias, x3))
    for tpw in (2, 3, 8):
        _setenv(monkeypatch, MMA_SKINNY_TPW=tpw)
        out = _linear_run(c, bias)
        assert torch.equal(out[0], base[0]), ("y", tpw)
        assert torch.equal(out[1], base[1]), ("gx", tpw)


def test_the_planner_s_own_three_tiles_per_wave(monkeypatch):
    """(78400, T = 5): 1535 workgroups at one tile per wave are three rounds of 512, 512 workgroups at three tiles are one - no variable."""
    N, T = 78400, 5
    assert R.tiles_per_wave(N, T) == 3 and R.tiles_per_wave(N - 64, T) == 1, "the shape no longer reaches the planner's multi-tile branch"
    c = _tower_case(N, T, 4, 3, tuple(SC[:1]))
    y, ga, _ = _tower_run(c, need_w=False)
    _tower_bars(c, y, ga, None, "natural plan")
    _setenv(monkeypatch, MMA_POST_TPW_ALL=1)
    y1, ga1, _ = _tower_run(c, need_w=False)
    assert torch.equal(y, y1) and torch.equal(ga, ga1)


def test_the_planner_s_own_two_tiles_per_wave_in_the_skinny_linear(monkeypatch):
    """K16 at 131136 rows: 513 workgroups at one tile per wave, 257 (one round) at two - no variable."""
    N = 131136
    assert R.tiles_per_wave(N, 1) == 2 and R.tiles_per_wave(N - 64, 1) == 1, "the shape no longer reaches the planner's multi-tile branch"
    c = _linear_case(N, 8, 5)
    out = _linear_run(c, True)
    _linear_bars(c, True, out, "natural plan")
    _setenv(monkeypatch, MMA_SKINNY_TPW=1)
    base = _linear_run(c, True)
    assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])


# ---- b. K15: node ranges, kf passes, the fallback reduction -----------------------------------------------------------------------
def _chunks(N, T):
    from mma_amd import _lib
    return _lib.query("mma_tower_post_gw_chunks", N, T)


def _gw_twice(c, tag):
    gw = _tower_run(c)[2]
    assert torch.equal(gw, _tower_run(c)[2]), "K15 sums in a fixed order: the same bits run after run (%s)" % tag
    R.assert_bar("gWo  %s %s" % ((c["N"], c["T"], c["KF"], c["O"], c["S"]), tag), gw, c["ref"]["gWo"], c["ref"]["mag_gw"], C_GW)
    return gw


def test_k15_node_ranges_of_64_and_192_nodes(monkeypatch):
    """(4097, T = 2): 17 chunks of four 64-node ranges by default.  MMA_POST_GW_WAVES=64: 32 waves per tower, 192-node ranges (twelve
    trips of the 16-node operand ring), 22 ranges in 6 chunks - the last workgroup has two idle waves whose range
    starts past N, its last working wave holds 65 rows.  63 is below the variable's floor: the default plan, bit for bit."""
    c = _tower_case(4097, 2, 36, 15, tuple(SC[:3]))
    assert _chunks(4097, 2) == 17
    gw_default = _gw_twice(c, "default plan")
    _setenv(monkeypatch, MMA_POST_GW_WAVES=64)
    assert _chunks(4097, 2) == 6
    _gw_twice(c, "MMA_POST_GW_WAVES=64")
    _setenv(monkeypatch, MMA_POST_GW_WAVES=63)
    assert _chunks(4097, 2) == 17
    assert torch.equal(_gw_twice(c, "MMA_POST_GW_WAVES=63"), gw_default)


@pytest.mark.parametrize("KF", [152, 164])
def test_k15_in_one_pass_of_ten_tiles_and_in_passes_of_five(KF, monkeypatch):
    """MMA_POST_GW_TILES=5 at S = 3 (G = 5 instead of 10: KF = 152 in two passes instead of one, 164 in three instead of two).  An
    output element's accumulator sees the same nodes in the same order and the four waves' tiles are added in the same order
    ((w0 + w1) + (w2 + w3)) under both, by reading the kernel: bit equality - and the GPU agrees."""
    c = _tower_case(130, 2, KF, 15, tuple(SC[:1] + SC[1:2] + SC[3:4]))
    gw10 = _gw_twice(c, "G=10")
    _setenv(monkeypatch, MMA_POST_GW_TILES=5)
    assert torch.equal(_gw_twice(c, "G=5"), gw10)


KF_PASSES = [(1, 160, 15, 3), (1, 164, 15, 3), (1, 512, 16, 3), (2, 84, 16, 4), (1, 320, 7, 5)]


@pytest.mark.parametrize("T,KF,O,S", KF_PASSES, ids=["one_full_pass", "second_pass_of_one_tile", "four_passes", "G5_two_passes", "G5_S5_four_passes"])
def test_k15_kf_passes(T, KF, O, S):
    c = _tower_case(130, T, KF, O, tuple(SC[:S]))
    _gw_twice(c, "kf passes")


def test_k15_fallback_reduction_through_col_sum(monkeypatch):
    """(66000, T = 1, KF = 8, S = 1) with MMA_POST_GW_WAVES=2048: 258 chunks of 256 partial columns - past mma_tower_post_gw_reduce's
    single-pass order, so _TowerPost.backward sums with dense.col_sum and permutes."""
    from mma_amd import dense
    c = _tower_case(66000, 1, 8, 3, tuple(SC[:1]))
    gw_default = _gw_twice(c, "default plan")
    _setenv(monkeypatch, MMA_POST_GW_WAVES=2048)
    assert _chunks(66000, 1) == 258
    seen, real = [], dense.col_sum
    monkeypatch.setattr(dense, "col_sum", lambda part, *a, **k: (seen.append(tuple(part.shape)), real(part, *a, **k))[1])
    gw = _gw_twice(c, "MMA_POST_GW_WAVES=2048")
    assert seen == [(258, 256)] * 2, seen
    R.assert_bar("gWo  fallback against the default plan", gw, gw_default.double(), c["ref"]["mag_gw"], 2 * C_GW)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 130])
def test_k15_small_node_counts(N):
    """A dropped or doubled row is 1/N of the sum: far above the bar here."""
    c = _tower_case(N, 2, 36, 15, tuple(SC[:3]))
    y, ga, gw = _tower_run(c)
    _tower_bars(c, y, ga, gw, "small N")


# ---- c. next to the LDS limit -------------------------------------------------------------------------------------------------------
LDS_SHAPES = [(2, 416, 16, 4), (2, 420, 16, 4), (1, 480, 16, 4), (1, 384, 7, 5), (1, 512, 16, 3)]


@pytest.mark.parametrize("T,KF,O,S", LDS_SHAPES, ids=["last_bf16x3_156KB", "fp32_fwd_154KB", "bwd_158KB", "bwd_159KB_S5", "KF512"])
def test_tower_shapes_next_to_the_lds_limit(T, KF, O, S):
    """What mma_tower_post_fits promises (and MMAConv's `factored` gate passes on): the last shape of the bf16-piece forward, the shapes
    behind it that take the exact-fp32 forward by default, K14 at 158 / 159 KB."""
    from mma_amd import dense
    assert dense.tower_post_fits(KF, S)
    c = _tower_case(130, T, KF, O, tuple(SC[:S]))
    y, ga, gw = _tower_run(c)
    _tower_bars(c, y, ga, gw, "LDS limit")


@pytest.mark.parametrize("K,O", [(512, 48), (384, 80), (416, 64), (320, 80)])
def test_skinny_linear_next_to_the_lds_limit(K, O):
    """K16 where _skinny_ok still says yes.  (384, 80) and (416, 64) have no bf16-piece form (their split weights are over 160 KB) and
    take the exact-fp32 forward by default.  (384, 80) is the regression case of that kernel's round-by-round summation: as one fp32
    chain over the 384 products its y sat at 3.116e-7 of sum|x||w| (torch fp32: 3.2e-7), over C_Y; summed per 32-column round 7.0e-8."""
    c = _linear_case(4160, K, O)
    out = _linear_run(c, True)                                   # asserts dense._skinny_ok
    _linear_bars(c, True, out, "LDS limit")


# ---- d. edge inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [None, "1"], ids=["default", "fp32_forward"])
@pytest.mark.parametrize("N,T,KF,O,scalers", [(1000, 5, 152, 15, tuple(SC[:1] + SC[1:2] + SC[3:4])), (4097, 3, 36, 16, tuple(SC))], ids=["zinc", "five_scalers"])
def test_tower_post_on_edge_rows(N, T, KF, O, scalers, exact, monkeypatch):
    """Rows spread over e^-6 .. e^6, a zero row, a row of one 1e30, a row of one 1e-30, a row with e^-14 .. 1 inside it, degrees 0, 1 and
    one hub of 10^6 - in agg and in the cotangent.  The per-element bars hold on every row, the tiny ones included."""
    c = _tower_case(N, T, KF, O, scalers, edges=True)
    _setenv(monkeypatch, MMA_POST_EXACT=exact)
    y, ga, gw = _tower_run(c)
    _tower_bars(c, y, ga, gw, "edge rows exact=%s" % exact)


@pytest.mark.parametrize("x3", [None, "0"], ids=["default", "fp32_forward"])
def test_skinny_linear_on_edge_rows(x3, monkeypatch):
    c = _linear_case(5000, 75, 75, edges=True)
    _setenv(monkeypatch, MMA_SKINNY_X3=x3)
    out = _linear_run(c, True)
    _linear_bars(c, True, out, "edge rows x3=%s" % x3)


# ---- e. isolation under poison: the raw entry points --------------------------------------------------------------------------------
def _codes(scalers):
    from mma_amd.functional import GR_SCALER
    from mma_amd._lib import host_codes
    return host_codes(GR_SCALER[s] for s in scalers)


def _pitched(src2d, pitch, rows_more, fill):
    buf = torch.full((src2d.shape[0] + rows_more, pitch), fill, device=DEV, dtype=torch.float32)
    buf[:src2d.shape[0], :src2d.shape[1]] = src2d
    return buf


def _untouched(buf, rows, cols):
    """Everything of a sentinel-filled output outside [:rows, :cols] still holds the sentinel."""
    return bool((buf[rows:] == SENT).all()) and bool((buf[:rows, cols:] == SENT).all())


def _raw_tower(agg, Wo, cot, rowptr, scalers, pad=(0, 0, 0), rows_more=0, want_gys=0):
    """K13, K14, K15 + the reduction through _lib.call on buffers with row pitches T*KF + pad[0], T*O + pad[1] (y), T*O + pad[2] (gy) and
    rows_more rows behind N; input padding NaN, output padding SENT.  -> dict(y, gagg, gWo, pre [, gys])."""
    from mma_amd import _lib
    from mma_amd._lib import call, ptr, stream_ptr
    N, T, KF = agg.shape
    O, S = Wo.shape[1], len(scalers)
    codes = _codes(scalers)
    nan = float("nan")
    KFp = int(_lib.lib().mma_tower_post_kfp(KF))
    Wa, Wb = torch.empty((T, KFp, S * 16), device=DEV), torch.empty((T, S * 16, KFp + 16), device=DEV)
    call("mma_tower_post_weights", ptr(Wo.contiguous()), T, O, S, KF, ptr(Wa), ptr(Wb), stream_ptr())
    pre = torch.full((N + rows_more, 8), SENT, device=DEV)
    call("mma_tower_post_pre", ptr(rowptr), ptr(pre), N, S, codes, AVG_LOG, AVG_LIN, stream_ptr())
    assert _untouched(pre, N, S), "mma_tower_post_pre wrote outside its (N, S) block"
    pre[N:] = nan
    pre[:, S:] = nan                                             # what the consumers must not read
    lda, ldy, ldg = T * KF + pad[0], T * O + pad[1], T * O + pad[2]
    a = _pitched(agg.reshape(N, T * KF), lda, rows_more, nan)
    g = _pitched(cot.reshape(N, T * O), ldg, rows_more, nan)
    y = torch.full((N + rows_more, ldy), SENT, device=DEV)
    call("mma_tower_post_fwd", ptr(a), lda, ptr(pre), ptr(Wa), ptr(y), ldy, N, T, KF, S, O, codes, AVG_LOG, AVG_LIN, stream_ptr())
    ga = torch.full((N + rows_more, lda), SENT, device=DEV)
    out = {}
    if want_gys:
        ldgs = T * S * 16 + want_gys
        gys = torch.full((N + rows_more, ldgs), SENT, device=DEV)
        call("mma_tower_post_bwd", ptr(g), ldg, ptr(pre), ptr(Wb), ptr(ga), lda, ptr(gys), ldgs, N, T, KF, S, O, codes, AVG_LOG, AVG_LIN, stream_ptr())
        assert _untouched(gys, N, T * S * 16), "gys: a store outside its (N, T*S*16) block"
        out["gys"] = gys[:N, :T * S * 16].reshape(N, T, S, 16)
    else:
        call("mma_tower_post_bwd", ptr(g), ldg, ptr(pre), ptr(Wb), ptr(ga), lda, None, 0, N, T, KF, S, O, codes, AVG_LOG, AVG_LIN, stream_ptr())
    n_chunks = _lib.query("mma_tower_post_gw_chunks", N, T)
    kfp16 = -(-KF // 16) * 16
    part = torch.full((n_chunks + 1, T * S * 16 * kfp16), SENT, device=DEV)
    call("mma_tower_post_gw", ptr(g), ldg, ptr(a), lda, ptr(pre), ptr(part), n_chunks, N, T, KF, S, O, codes, AVG_LOG, AVG_LIN, stream_ptr())
    gWo = torch.full((T * O * S * KF + 64,), SENT, device=DEV)
    call("mma_tower_post_gw_reduce", ptr(part), n_chunks, T, S, O, KF, ptr(gWo), stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(y, N, T * O), "K13: a store outside the (N, T*O) block of y"
    assert _untouched(ga, N, T * KF), "K14: a store outside the (N, T*KF) block of gagg"
    assert bool((part[n_chunks:] == SENT).all()) and not bool((part[:n_chunks] == SENT).any()), "K15: partial tiles"
    assert bool((gWo[T * O * S * KF:] == SENT).all()), "the reduction wrote past gWo"
    out.update(y=y[:N, :T * O].contiguous(), gagg=ga[:N, :T * KF].reshape(N, T, KF).contiguous(), gWo=gWo[:T * O * S * KF].view(T, O, S * KF),
               pre=pre[:N, :S].contiguous())
    return out


def _raw_case(N, T, KF, O, S, seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 7, (N,), generator=g)
    return (torch.randn(N, T, KF, generator=g).to(DEV), (torch.randn(T, O, S * KF, generator=g) / np.sqrt(S * KF)).to(DEV),
            torch.randn(N, T * O, generator=g).to(DEV), R.rowptr_of(deg).to(DEV), deg)


@pytest.mark.parametrize("exact", [None, "1"], ids=["bf16x3_forward", "fp32_forward"])
@pytest.mark.parametrize("KF,pad", [(36, (4, 3, 5)), (36, (1, 1, 1)), (37, (1, 3, 5))], ids=["vec4_pitch", "dword_pitch", "KF37_raw_only"])
@pytest.mark.parametrize("N", [65, 321])
def test_row_strided_buffers_with_poisoned_padding(N, KF, pad, exact, monkeypatch):
    """K13 (both forms), K14 and K15 on row-strided buffers (lda > T*KF, ldy > T*O, ldg > T*O, 64 rows behind N): every pad column and
    pad row of the inputs is NaN, of the outputs a sentinel.  The kernels load from clamped addresses and zero by selects - a select
    that lets a pad value through shows as a NaN, a store one column or one row too far as a changed sentinel (checked inside
    _raw_tower).  Equal to the contiguous run bit for bit.  KF = 37 (no float4 rows) is a shape only the raw entry reaches."""
    T, O, scalers = 3, 15, SC[:3]
    _setenv(monkeypatch, MMA_POST_EXACT=exact)
    agg, Wo, cot, rowptr, deg = _raw_case(N, T, KF, O, 3, N + KF)
    flat = _raw_tower(agg, Wo, cot, rowptr, scalers)
    wide = _raw_tower(agg, Wo, cot, rowptr, scalers, pad=pad, rows_more=64)
    ref = R.tower_post64(agg.cpu(), Wo.cpu(), R.pre64(deg, scalers, AVG_LOG, AVG_LIN), cot.cpu())
    for k, c in (("y", C_Y), ("gWo", C_GW)):
        assert not torch.isnan(wide[k]).any(), k
        assert torch.equal(wide[k], flat[k]), k
        R.assert_bar("%s raw N=%d KF=%d" % (k, N, KF), flat[k], ref[k], ref["mag_" + {"y": "y", "gWo": "gw"}[k]], c)
    assert not torch.isnan(wide["gagg"]).any() and torch.equal(wide["gagg"], flat["gagg"])
    R.assert_ga_bar("gagg raw N=%d KF=%d" % (N, KF), flat["gagg"], R.tower_post32(agg, Wo, flat["pre"], cot), ref["gagg"], ref["mag_ga"], 3)


def _raw_linear(x, W, b, cot, pad=(0, 0, 0), rows_more=0):
    """The K16 trio through _lib.call: ldx = K + pad[0], ldy = O + pad[1], ldg = O + pad[2]; input padding NaN, output padding SENT."""
    from mma_amd import _lib
    from mma_amd._lib import call, ptr, stream_ptr
    (N, K), O = x.shape, W.shape[0]
    S, nan = -(-O // 16), float("nan")
    kfp = int(_lib.lib().mma_tower_post_kfp(K))
    Wa, Wb = torch.empty((kfp, S * 16), device=DEV), torch.empty((S * 16, kfp + 16), device=DEV)
    call("mma_skinny_linear_weights", ptr(W), O, K, ptr(Wa), ptr(Wb), stream_ptr())
    ldx, ldy, ldg = K + pad[0], O + pad[1], O + pad[2]
    xb, gb_in = _pitched(x, ldx, rows_more, nan), _pitched(cot, ldg, rows_more, nan)
    y = torch.full((N + rows_more, ldy), SENT, device=DEV)
    call("mma_skinny_linear_fwd", ptr(xb), ldx, ptr(Wa), ptr(b), None, 0, ptr(y), ldy, N, K, O, stream_ptr())
    gx = torch.full((N + rows_more, ldx), SENT, device=DEV)
    call("mma_skinny_linear_bwd_dx", ptr(gb_in), ldg, ptr(Wb), ptr(gx), ldx, N, K, O, stream_ptr())
    n_part = _lib.query("mma_skinny_linear_gw_part", N, K, O)
    part = torch.empty(n_part, device=DEV)
    gw, gb = torch.full((O * K + 64,), SENT, device=DEV), torch.full((O + 64,), SENT, device=DEV)
    call("mma_skinny_linear_gw", ptr(gb_in), ldg, ptr(xb), ldx, ptr(part), n_part, ptr(gw), ptr(gb), N, K, O, stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(y, N, O), "K16 forward: a store outside the (N, O) block"
    assert _untouched(gx, N, K), "K16 dL/dx: a store outside the (N, K) block"
    assert bool((gw[O * K:] == SENT).all()) and bool((gb[O:] == SENT).all()), "K16 gradient: a store past gw / gb"
    return y[:N, :O].contiguous(), gx[:N, :K].contiguous(), gw[:O * K].view(O, K), gb[:O]


@pytest.mark.parametrize("x3", [None, "0"], ids=["bf16x3_forward", "fp32_forward"])
@pytest.mark.parametrize("K,pad", [(36, (4, 3, 5)), (37, (1, 3, 5))], ids=["vec4_pitch", "K37"])
@pytest.mark.parametrize("N", [65, 321])
def test_skinny_linear_on_row_strided_buffers_with_poisoned_padding(N, K, pad, x3, monkeypatch):
    """The K16 trio (forward, dL/dx, weight + bias gradient) under the same poison, O = 45: three 16-row tiles, the last one partial."""
    O = 45
    _setenv(monkeypatch, MMA_SKINNY_X3=x3)
    g = torch.Generator().manual_seed(N + K)
    x, W = torch.randn(N, K, generator=g).to(DEV), (torch.randn(O, K, generator=g) / 6).to(DEV)
    b, cot = torch.randn(O, generator=g).to(DEV), torch.randn(N, O, generator=g).to(DEV)
    flat = _raw_linear(x, W, b, cot)
    wide = _raw_linear(x, W, b, cot, pad=pad, rows_more=64)
    ref = R.linear64(x.cpu(), W.cpu(), b.cpu(), cot.cpu())
    for got_w, got_f, k, m, c in zip(wide, flat, ("y", "gx", "gW", "gb"), ("mag_y", "mag_gx", "mag_gw", "mag_gb"), (C_Y, None, C_GW, C_GW)):
        assert not torch.isnan(got_w).any(), k
        assert torch.equal(got_w, got_f), k
        if c is None:
            R.assert_ga_bar("gx raw K16 N=%d K=%d" % (N, K), got_f, cot @ W, ref[k], ref[m], 3)
        else:
            R.assert_bar("%s raw K16 N=%d K=%d" % (k, N, K), got_f, ref[k], ref[m], c)


@pytest.mark.parametrize("exact", [None, "1"], ids=["bf16x3_forward", "fp32_forward"])
def test_a_tower_does_not_see_its_neighbour(exact, monkeypatch):
    """agg of tower 1 all inf, and - separately - the gradient of tower 1's outputs all NaN: y, gagg and gWo of towers 0 and 2 keep
    every bit of the clean run."""
    N, T, KF, O, scalers = 321, 3, 36, 15, SC[:3]
    _setenv(monkeypatch, MMA_POST_EXACT=exact)
    agg, Wo, cot, rowptr, _ = _raw_case(N, T, KF, O, 3, 77)
    clean = _raw_tower(agg, Wo, cot, rowptr, scalers)
    bad_agg = agg.clone(); bad_agg[:, 1, :] = float("inf")
    bad_cot = cot.clone(); bad_cot.view(N, T, O)[:, 1, :] = float("nan")
    for what, run in (("agg[:, 1] = inf", _raw_tower(bad_agg, Wo, cot, rowptr, scalers)), ("gy[:, 1] = NaN", _raw_tower(agg, Wo, bad_cot, rowptr, scalers))):
        for t in (0, 2):
            assert torch.equal(run["y"].view(N, T, O)[:, t], clean["y"].view(N, T, O)[:, t]), (what, "y", t)
            assert torch.equal(run["gagg"][:, t], clean["gagg"][:, t]), (what, "gagg", t)
            assert torch.equal(run["gWo"][t], clean["gWo"][t]), (what, "gWo", t)
    assert not torch.isfinite(_raw_tower(bad_agg, Wo, cot, rowptr, scalers)["y"].view(N, T, O)[:, 1]).any(), "the poison did not reach tower 1"


@pytest.mark.parametrize("exact", [None, "1"], ids=["bf16x3_forward", "fp32_forward"])
def test_a_node_does_not_see_its_neighbour(exact, monkeypatch):
    """One row of agg all NaN, and - separately - one row of the gradient: only that node's y / gagg are NaN, every other row keeps
    every bit (a node is a column of the matrix-core tiles; rows past N are loaded from row N - 1)."""
    N, T, KF, O, scalers = 130, 2, 36, 15, SC[:3]
    _setenv(monkeypatch, MMA_POST_EXACT=exact)
    agg, Wo, cot, rowptr, _ = _raw_case(N, T, KF, O, 3, 78)
    clean = _raw_tower(agg, Wo, cot, rowptr, scalers)
    for row in (70, N - 1):
        others = [n for n in range(N) if n != row]
        bad = agg.clone(); bad[row] = float("nan")
        run = _raw_tower(bad, Wo, cot, rowptr, scalers)
        assert torch.isnan(run["y"][row]).all() and torch.equal(run["y"][others], clean["y"][others]), row
        assert torch.equal(run["gagg"], clean["gagg"]), row
        bad = cot.clone(); bad[row] = float("nan")
        run = _raw_tower(agg, Wo, bad, rowptr, scalers)
        assert torch.isnan(run["gagg"][row]).all() and torch.equal(run["gagg"][others], clean["gagg"][others]), row
        assert torch.equal(run["y"], clean["y"]), row


def test_fp32_forward_keeps_an_infinity_an_infinity(monkeypatch):
    """The exact-fp32 forward with one +inf in the LAST column of a tower (KF = 36: the 28 columns up to the 64-column round are loaded
    from the clamped address of the last quad and zeroed by a select - their weights are zero, but 0 x inf is not): that node's outputs
    are the infinities float64 gives, not NaN, and nothing else changes.  (The bf16-piece forward cannot be asked this: its split turns
    an infinity into a NaN piece by itself, inf - inf.)"""
    N, T, KF, O, scalers = 65, 2, 36, 15, SC[:1]
    _setenv(monkeypatch, MMA_POST_EXACT=1)
    agg, Wo, cot, rowptr, deg = _raw_case(N, T, KF, O, 1, 79)
    clean = _raw_tower(agg, Wo, cot, rowptr, scalers)["y"].view(N, T, O)
    bad = agg.clone(); bad[5, 1, KF - 1] = float("inf")
    y = _raw_tower(bad, Wo, cot, rowptr, scalers)["y"].view(N, T, O)
    want = R.tower_post64(bad.cpu(), Wo.cpu(), R.pre64(deg, scalers, AVG_LOG, AVG_LIN), cot.cpu())["y"].view(N, T, O)
    assert torch.isinf(want[5, 1]).all() and torch.equal(y[5, 1].cpu().double(), want[5, 1])
    y[5, 1] = clean[5, 1]
    assert torch.equal(y, clean)
    # K16's fp32 forward: the same select
    g = torch.Generator().manual_seed(80)
    x, W, b = torch.randn(N, KF, generator=g).to(DEV), torch.randn(45, KF, generator=g).to(DEV), torch.randn(45, generator=g).to(DEV)
    _setenv(monkeypatch, MMA_SKINNY_X3=0, MMA_POST_EXACT=None)
    clean = _raw_linear(x, W, b, cot[:, :1].expand(N, 45).contiguous())[0]
    bad = x.clone(); bad[5, KF - 1] = float("inf")
    y = _raw_linear(bad, W, b, cot[:, :1].expand(N, 45).contiguous())[0]
    assert torch.equal(y[5], torch.sign(W[:, KF - 1]) * float("inf"))
    y[5] = clean[5]
    assert torch.equal(y, clean)


@pytest.mark.parametrize("N,T,KF,O,S", [(321, 3, 36, 15, 3), (65, 2, 100, 7, 5), (130, 1, 4, 16, 1)])
def test_gys_the_optional_second_output_of_k14(N, T, KF, O, S):
    """mma_tower_post_bwd(..., gys, ldgs): gys[n, t, q, o] = pre[n, q] * gy[n, t*O + o] - the fp32 product, exactly, pre from
    mma_tower_post_pre -, zeros in the padded outputs o >= O, nothing outside the (N, T*S*16) block of a wider buffer (checked inside
    _raw_tower), and gagg as without it."""
    agg, Wo, cot, rowptr, _ = _raw_case(N, T, KF, O, S, N + S)
    plain = _raw_tower(agg, Wo, cot, rowptr, SC[:S])
    both = _raw_tower(agg, Wo, cot, rowptr, SC[:S], rows_more=64, want_gys=7)
    want = torch.zeros((N, T, S, 16), device=DEV)
    want[..., :O] = both["pre"].view(N, 1, S, 1) * cot.view(N, T, 1, O)
    assert torch.equal(both["gys"], want)
    assert torch.equal(both["gagg"], plain["gagg"])


@pytest.mark.parametrize("scalers", [tuple(SC), tuple(SC[::-1]), tuple(SC[1:4])], ids=["five", "five_reversed", "three"])
def test_scaler_table_against_float64(scalers):
    """mma_tower_post_pre against pre64 with degrees 0 (clamped to 1), 1, 2, 10^6.  Yardstick: torch's own fp32 expression on the GPU;
    bar: 2 * its error + 2^-23, relative per element.  The eight-float row holds S values: columns q >= S of a sentinel-filled table
    stay untouched."""
    from mma_amd._lib import call, ptr, stream_ptr
    S = len(scalers)
    deg = torch.tensor([0, 1, 2, 10 ** 6] + list(range(3, 300)), dtype=torch.int64)
    N = deg.numel()
    rowptr = R.rowptr_of(deg).to(DEV)
    pre = torch.full((N + 3, 8), SENT, device=DEV)
    call("mma_tower_post_pre", ptr(rowptr), ptr(pre), N, S, _codes(scalers), AVG_LOG, AVG_LIN, stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(pre, N, S)
    truth = R.pre64(deg, scalers, AVG_LOG, AVG_LIN)
    assert torch.equal(truth[0], truth[1]), "degree 0 counts as 1"
    e_got = R.err_over_mag(pre[:N, :S], truth, truth.abs())
    e_f32 = R.err_over_mag(R.pre64(deg.to(DEV), scalers, AVG_LOG, AVG_LIN, dtype=torch.float32), truth, truth.abs())
    print("PRE %-44s e_got %.3e  e_f32 %.3e" % (scalers, e_got, e_f32))
    assert e_got <= 2 * e_f32 + 2.0 ** -23, (e_got, e_f32)
