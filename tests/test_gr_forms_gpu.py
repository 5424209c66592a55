"""K3 / K4 (gr_fused.hip) in the forms the layer's usual shapes do not reach, against the plain reference of tests/gr_ref.py.  Every case
first asserts, with functional.gr_plan, which kernels its calls take.

A. segments of 256 edges and more: the saved arg moves from a byte per column to an int32 row of the side table;
B. the block kernels' LDS-driven nb ladder at real widths, and calls whose forward and backward take different forms;
C. the fused message off the layer's path: VEC = 1, odd pitches and bases, by_pos 0 / 1, a categorical Z table in every kernel family;
D. the grid-stride loops of the wave-per-node and the flat kernels.

Bars: golden_util.check_close as it is - strict for given messages (multiples of 0.25: their sums are exact), the float64-noise bar
for sums of fused messages; exact equality for min / max values, empty targets, args and 0 / 1 gradient patterns."""
import numpy as np
import pytest
import torch

import gr_ref as R
from golden_util import check_close
from test_segment_kernels_gpu import gr_targets

pytestmark = pytest.mark.gpu

ALL_AGGS = ["sum", "mean", "min", "max", "var", "std"]
FUSED_AGGS = ["sum", "mean", "min", "max"]


def quarters(rng, shape):
    return rng.integers(-4, 5, shape).astype(np.float32) * 0.25


def block_of(a, T, F, K, S, k, q=0):
    """aggregator k's block of scaler q of an (N, T, S*K*F) output"""
    return np.asarray(a).reshape(-1, T, S, K, F)[:, :, q, k]


# ---- shared checks ---------------------------------------------------------------------------------------------------------------------

def assert_empty_targets(L, r, ref, what):
    """Targets without an edge hold the reference's values bit for bit: 0, or the float32 sqrt(1e-5) of std times the scalers of the
    clamped degree 1; their dL/dU rows are 0."""
    empty = L.deg == 0
    got, want = r.out.numpy()[empty], ref["out32"][empty]
    print("%s: %d empty targets, max |got - want| %.3g" % (what, int(empty.sum()), float(np.abs(got - want).max()) if got.size else 0.0))
    assert np.array_equal(got, want), what + ": empty targets differ from the reference's 0 / sqrt(1e-5)"
    for gu, gw in zip(r.gU, ref["gU32"]):
        assert gu is None or (np.array_equal(gu[empty], gw[empty]) and (gu[empty] == 0).all()), what + ": dL/dU rows of empty targets"


def check_given(L, T, F, aggs, scalers, inputs, expect, with_list=True, what=""):
    """Given messages: out and dL/dinputs strict, min / max blocks, args and the 0 / 1 patterns exact.  Returns what the ways of running
    one degree list must agree on."""
    D, K, S = T * F, len(aggs), len(scalers)
    rng = np.random.default_rng(L.E + D)
    gouts = [rng.standard_normal((L.N, T, S * K * F)).astype(np.float32)]
    ext = [k for k, a in enumerate(aggs) if a in ("min", "max")]
    gouts += [R.onehot_gout(L.N, T, F, K, S, k) for k in ext]
    ref = R.reference(L, inputs, None, T, F, aggs, scalers, gouts)
    r = R.run(L, T, F, aggs, scalers, gouts, inputs=inputs, with_list=with_list, expect=expect)
    check_close(r.out, ref["out32"], None, None, what=what + " out")
    check_close(torch.from_numpy(r.gmsg[0]), ref["gmsg32"][0], None, None, what=what + " dL/dinputs")
    assert_empty_targets(L, r, ref, what)
    same = {}
    for i, k in enumerate(ext):
        got_blk, want_blk = block_of(r.out.numpy(), T, F, K, S, k), block_of(ref["out32"], T, F, K, S, k)
        assert np.array_equal(got_blk, want_blk), "%s: the %s block is not the oracle's bit for bit" % (what, aggs[k])
        assert np.array_equal(r.gmsg[1 + i], ref["gmsg32"][1 + i]), "%s: 0/1 gradient pattern of %s" % (what, aggs[k])
        want = R.arg_offsets(L, inputs, aggs[k])
        assert np.array_equal(want, R.arg_offsets_vectorised(L, inputs, aggs[k]))
        a8, side = (r.amin, r.amin_side) if aggs[k] == "min" else (r.amax, r.amax_side)
        R.assert_saved_args(L, D, a8, side, want, "%s %s" % (what, aggs[k]))
        same[aggs[k]] = (got_blk, a8, side, r.gmsg[1 + i][L.perm])
    return same


def check_fused(L, T, F, aggs, scalers, p, expect, rng, Z="rows", by_pos=True, with_list=True, want_msg=None, what="", **kw):
    """drop(U[i] + V[j] + Z[r]): out, gmsg and gU at the float64-noise bar, the min / max blocks, their args and 0 / 1 patterns exact,
    NaN-filled pitch columns untouched.  Z: "rows" (E, D), "table" (4 rows and a uint8 index) or None; want_msg (E, D): Z rows are
    chosen so that the message before dropout is exactly this.  Returns the run and the reference."""
    D, K, S = T * F, len(aggs), len(scalers)
    U, V = quarters(rng, (L.N, D)), quarters(rng, (L.N, D))
    Zr = zidx = None
    if Z == "rows":
        Zr = quarters(rng, (L.E, D)) if want_msg is None else (want_msg - (V[L.src] + U[L.dst])).astype(np.float32)
    elif Z == "table":
        Zr, zidx = quarters(rng, (4, D)), rng.integers(0, 4, L.E).astype(np.uint8)
    seed = 0x5EED + D
    s = R.fused_sum(L, U, V, Zr, zidx)
    if want_msg is not None:
        assert np.array_equal(s, want_msg)
    fac = R.drop_factor(p, seed, L.E, D)
    h = s if fac is None else s * fac
    gouts = [rng.standard_normal((L.N, T, S * K * F)).astype(np.float32)]
    ext = [k for k, a in enumerate(aggs) if a in ("min", "max")]
    gouts += [R.onehot_gout(L.N, T, F, K, S, k) for k in ext]
    ref = R.reference(L, s, fac, T, F, aggs, scalers, gouts)
    ref["bound"] = R.node_bounds(L, T, F, aggs, scalers, gouts[0], p) if kw.get("row_max") else None
    r = R.run(L, T, F, aggs, scalers, gouts, U=U, V=V, Z=Zr, zidx=zidx, by_pos=by_pos, p=p, seed=seed, with_list=with_list, expect=expect,
              **kw)
    rows = L.perm if by_pos else np.arange(L.E)                      # gmsg rows: positions or original ids
    check_close(r.out, ref["out32"], None, None, what=what + " out", signed_sum=True, truth=ref["out64"])
    check_close(torch.from_numpy(r.gmsg[0]), ref["gmsg32"][0][rows], None, None, what=what + " gmsg", signed_sum=True,
                truth=ref["gmsg64"][0][rows])
    check_close(torch.from_numpy(r.gU[0]), ref["gU32"][0], None, None, what=what + " gU", signed_sum=True, truth=ref["gU64"][0])
    assert_empty_targets(L, r, ref, what)
    for i, k in enumerate(ext):
        assert np.array_equal(block_of(r.out.numpy(), T, F, K, S, k), block_of(ref["out32"], T, F, K, S, k)), \
            "%s: the %s block is not the oracle's bit for bit" % (what, aggs[k])
        assert np.array_equal(r.gmsg[1 + i], ref["gmsg32"][1 + i][rows]), "%s: 0 / scale gradient pattern of %s" % (what, aggs[k])
        a8, side = (r.amin, r.amin_side) if aggs[k] == "min" else (r.amax, r.amax_side)
        R.assert_saved_args(L, D, a8, side, R.arg_offsets(L, h, aggs[k]), "%s %s" % (what, aggs[k]))
    for j in range(len(gouts)):
        assert r.gmsg_pad[j] is None or np.isnan(r.gmsg_pad[j]).all(), what + ": pitch columns of gmsg were written"
        assert np.isnan(r.gu_pad[j]).all(), what + ": columns of the gU buffer beyond D were written"
    return r, ref


# ---- A. long segments and the side table ----------------------------------------------------------------------------------------------

LONG_LISTS = {
    # segment starts 255, 511, 768 (a multiple of 256), 1198, 1713, 1969 -> side rows 1, 2, 3, 5, 7, 8
    "mixed": ([255, 256, 257, 0, 300, 64, 65, 1, 512, 3, 256, 256], [1, 2, 3, 5, 7, 8]),
    # a long segment at position 0 -> side row 0; the 255-edge segment keeps bytes (largest offset 254)
    "from0": ([256, 256, 1, 255, 1024], [0, 1, 3]),
}
WIDTHS_A = [(1, 1), (3, 5), (2, 8), (1, 68), (5, 52)]      # lpr 1; VEC 1, 16 lanes; 2 quads; 17 quads -> 32 lanes; 65 quads -> 16 x 5


def with_filler(deg):
    """deg followed by enough degree 1..3 nodes that E <= 16 N"""
    deg = list(deg)
    fill = []
    while sum(deg) + sum(fill) > 16 * (len(deg) + len(fill)):
        fill.append(1 + len(fill) % 3)
    return deg + fill


def planted(L, n_hub, D, rng):
    """(E_hub, D) messages in POSITION order for the first n_hub nodes: multiples of 0.25 in [-1, 1], and in every segment of 255 edges
    and more: column 0 a unique maximum at the last offset and a unique minimum at offset 0, column 1 all equal (arg = offset 0), column
    2 a unique maximum at offset 255 (the byte sentinel 0xFF), column 3 a unique minimum at offset 256 (where a byte wraps to 0)."""
    E_hub = int(L.rowptr[n_hub])
    H = quarters(rng, (E_hub, D))
    for n in range(n_hub):
        b, d = int(L.rowptr[n]), int(L.deg[n])
        if d < 255:
            continue
        H[b + d - 1, 0], H[b, 0] = 2.0, -2.0
        if D > 1:
            H[b:b + d, 1] = 0.5
        if D > 2 and d > 255:
            H[b + 255, 2] = 2.0
        if D > 3 and d > 256:
            H[b + 256, 3] = -2.0
    return H


def ways(name, rng_seed):
    """The three ways of running a degree list: alone (E > 16 N: the wave kernel takes everything), with filler nodes and the long-node
    list, with filler nodes and no list."""
    deg, side_rows = LONG_LISTS[name]
    La = R.Layout(deg, np.random.default_rng(rng_seed))
    Lb = R.Layout(with_filler(deg), np.random.default_rng(rng_seed + 1))
    assert La.E > 16 * La.N and Lb.E <= 16 * Lb.N
    long = np.nonzero(La.deg >= 256)[0]
    assert ((La.rowptr[long] + 255) // 256).tolist() == side_rows and ((Lb.rowptr[long] + 255) // 256).tolist() == side_rows
    return La, Lb, len(deg)


def hub_messages(L, Hp, rng):
    """(E, D) by original edge id: the hub segments hold Hp (position order), the filler edges random quarters"""
    h = quarters(rng, (L.E, Hp.shape[1]))
    h[L.perm[:len(Hp)]] = Hp
    return h


@pytest.mark.parametrize("name", list(LONG_LISTS))
@pytest.mark.parametrize("T,F", WIDTHS_A)
def test_long_segments_given_messages(name, T, F):
    """All six aggregators x {identity, amplification, attenuation} on given messages; the three ways agree bit for bit in the min / max
    blocks, the saved args and the 0 / 1 patterns of the hub nodes."""
    D = T * F
    La, Lb, n_hub = ways(name, 100 + D)
    rng = np.random.default_rng(D)
    Hp = planted(La, n_hub, D, rng)
    scalers = ["identity", "amplification", "attenuation"]
    vec = 4 if F % 4 == 0 else 1
    runs = [(La, True, dict(fwd="none", bwd="none", second="wave", vec=vec)),
            (Lb, True, dict(fwd="flat", bwd="flat", second="list", vec=vec)),           # var / std: no block kernel
            (Lb, False, dict(fwd="flat", bwd="flat", second="wave-long", vec=vec))]
    E_hub = len(Hp)
    first = None
    for L, with_list, expect in runs:
        same = check_given(L, T, F, ALL_AGGS, scalers, hub_messages(L, Hp, np.random.default_rng(7)), expect, with_list,
                           what="%s %dx%d %s" % (name, T, F, expect["second"]))
        long = np.nonzero(La.deg >= 256)[0]
        hub = {a: (blk[:n_hub], a8[:n_hub][(La.deg > 0) & (La.deg < 256)], side[(La.rowptr[long] + 255) // 256], pat[:E_hub])
               for a, (blk, a8, side, pat) in same.items()}
        if first is None:
            first = hub
        else:
            for a in hub:
                for x, y in zip(hub[a], first[a]):
                    assert np.array_equal(x, y), "%s: the %s pass disagrees with the wave-only run on the hub nodes" % (a, expect["second"])


@pytest.mark.parametrize("name", list(LONG_LISTS))
@pytest.mark.parametrize("T,F", WIDTHS_A)
@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
def test_long_segments_fused_messages(name, T, F, p):
    """sum, mean, min, max on drop(U + V + Z) with the planted messages; the list pass and the wave pass behind the same first kernel
    agree bit for bit in everything."""
    D = T * F
    La, Lb, n_hub = ways(name, 200 + D)
    rng = np.random.default_rng(D + int(p * 10))
    Hp = planted(La, n_hub, D, rng)
    scalers = ["identity", "amplification"]
    vec = 4 if F % 4 == 0 else 1
    first = "block" if vec == 4 else "flat"
    check_fused(La, T, F, FUSED_AGGS, scalers, p, dict(fwd="none", bwd="none", second="wave", vec=vec), rng,
                want_msg=hub_messages(La, Hp, np.random.default_rng(8)), what="%s %dx%d p=%g wave" % (name, T, F, p))
    res = []
    for with_list in (True, False):
        expect = dict(fwd=first, bwd=first, second="list" if with_list else "wave-long", vec=vec)
        r, _ = check_fused(Lb, T, F, FUSED_AGGS, scalers, p, expect, np.random.default_rng(D), with_list=with_list,
                           want_msg=hub_messages(Lb, Hp, np.random.default_rng(8)), what="%s %dx%d p=%g %s" % (name, T, F, p, expect["second"]))
        res.append(r)
    a, b = res
    assert torch.equal(a.out, b.out) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a.gmsg + a.gU, b.gmsg + b.gU))
    assert np.array_equal(a.amin, b.amin) and np.array_equal(a.amax, b.amax)
    assert np.array_equal(a.amax_side, b.amax_side) and np.array_equal(a.amin_side, b.amin_side)


# ---- B. the LDS ladder with real layouts, and form hand-offs ---------------------------------------------------------------------------

_B_LAYOUT = []


def b_layout():
    if not _B_LAYOUT:
        _B_LAYOUT.append(R.Layout(gr_targets(), np.random.default_rng(384)))
    return _B_LAYOUT[0]


def check_row_maxima(L, r, bwd, bound, by_pos=True):
    """What include/mma_amd.h and test_gr_gpu.py::test_backward_row_maxima_bound_the_rows_they_stand_for state of K4's row maxima: every
    entry is >= max |row|; dL/dU entries are within 2^-7 above the maximum; the flat kernel and the wave-per-node pass (segments above
    64 edges) store the maxima themselves; the block kernel gives all rows of a node ONE bound, the documented one: the keep scale times
    |c_all| + |c_min| + |c_max| of the node's worst column, its upper 16 bits rounded up (within 2^-7 above) - `bound` = (value, slack)
    per node from gr_ref.node_bounds in float64, the slack being the fp32 rounding of the coefficient sums.  (That test's "within a
    factor 8 for all but 2 % of the rows" is the same statement in the statistics of its molecule batch; the exact bound replaces it.)"""
    gm, gu, rm, ru = r.gmsg[0], r.gU[0], r.rm_msg[0], r.rm_u[0]
    true_m, true_u = np.abs(gm).max(1), np.abs(gu).max(1)
    if not by_pos:
        true_m, rm = true_m[L.perm], rm[L.perm]                      # position order
    assert not np.isnan(gm).any() and (rm >= true_m).all(), "a message-gradient bound below its row's maximum"
    assert (ru >= true_u).all() and (ru <= true_u * (1 + 2.0 ** -7)).all(), "dL/dU row maxima: upper bounds within 2^-7"
    long_rows = L.deg[L.seg] > 64                                    # positions of the long segments' edges
    exact = long_rows if bwd == "block" else np.ones(L.E, bool)
    assert np.array_equal(rm[exact], true_m[exact]) and np.array_equal(ru[L.deg > 64], true_u[L.deg > 64]), \
        "the flat kernel and the wave-per-node pass store max |row| itself"
    if bwd == "block":
        value, slack = bound[0][L.seg][~long_rows], bound[1][L.seg][~long_rows]
        got = rm[~long_rows].astype(np.float64)
        print("block bounds / documented bound: %.6f .. %.6f over %d rows" % (
            float((got / value).min()), float((got / value).max()), len(got)))
        assert (got >= value - slack).all() and (got <= (value + slack) * (1 + 2.0 ** -7)).all(), \
            "the block kernel's bound is not scale * max_c (|c_all| + |c_min| + |c_max|) rounded up within 2^-7"


LADDER_B = [(212, 16), (216, 8), (428, 8), (432, 4), (856, 4), (860, 2), (1716, 2), (1720, None)]      # D, nb (None: the flat kernel)


@pytest.mark.parametrize("D,nb", LADDER_B)
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_nb_ladder_min_max(D, nb, wide, p, monkeypatch):
    """[min, max] x 4 scalers (K * S = 8, two LDS planes both ways) at the last width of every nb step and the first past it, as D / 4
    towers of F = 4 and as one tower of F = D (the two extremes of the column decodes)."""
    monkeypatch.delenv("MMA_GR_NB", raising=False)
    T, F = (1, D) if wide else (D // 4, 4)
    L = b_layout()
    form = "block" if nb else "flat"
    expect = dict(fwd=form, bwd=form, second="list", vec=4, nb_fwd=nb or 16, nb_bwd=nb or 16)
    r, ref = check_fused(L, T, F, ["min", "max"], ["identity", "amplification", "attenuation", "linear"], p, expect,
                       np.random.default_rng(D + wide), what="ladder D=%d F=%d p=%g" % (D, F, p), pad_g=4, pad_gu=4, row_max=True)
    check_row_maxima(L, r, expect["bwd"], ref["bound"])


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_forward_flat_backward_block(p, monkeypatch):
    """[sum, mean, min, max] x 2 scalers at D = 1224: the forward's four planes do not fit the LDS budget (flat), the backward's three do
    at nb = 2 (block) - K4's block kernel reads the arg bytes K3's flat kernel wrote."""
    monkeypatch.delenv("MMA_GR_NB", raising=False)
    L = b_layout()
    expect = dict(fwd="flat", bwd="block", second="list", vec=4, nb_fwd=16, nb_bwd=2)
    r, ref = check_fused(L, 6, 204, FUSED_AGGS, ["identity", "attenuation"], p, expect, np.random.default_rng(1224),
                       what="flat -> block p=%g" % p, pad_g=4, pad_gu=4, row_max=True)
    check_row_maxima(L, r, expect["bwd"], ref["bound"])


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_forward_block_backward_flat(p, monkeypatch):
    """[sum, mean, max] x 3 scalers (K * S = 9) at D = 612: block forward at nb = 4, flat backward, at a real LDS offset."""
    monkeypatch.delenv("MMA_GR_NB", raising=False)
    L = b_layout()
    expect = dict(fwd="block", bwd="flat", second="list", vec=4, nb_fwd=4, nb_bwd=16)
    r, ref = check_fused(L, 3, 204, ["sum", "mean", "max"], ["identity", "amplification", "linear"], p, expect,
                       np.random.default_rng(612), what="block -> flat p=%g" % p, pad_g=4, pad_gu=4, row_max=True)
    check_row_maxima(L, r, expect["bwd"], ref["bound"])


# ---- C. the fused form off the layer's path --------------------------------------------------------------------------------------------

def small_graph():
    """40 nodes, E <= 16 N, a 70-edge hub (the list pass)"""
    deg = np.random.default_rng(40).integers(0, 5, 40)
    deg[7] = 70
    return R.Layout(deg, np.random.default_rng(41))


def tiny_graph():
    """6 nodes, E > 16 N: the wave kernel takes everything"""
    return R.Layout([20, 30, 0, 17, 25, 40], np.random.default_rng(6))


def c_expect(L, vec, block=True):
    if L.E > 16 * L.N:
        return dict(fwd="none", bwd="none", second="wave", vec=vec)
    form = "block" if vec == 4 and block else "flat"
    return dict(fwd=form, bwd=form, second="list", vec=vec)


GRAPHS_C = {"small": small_graph, "tiny": tiny_graph}
SC2 = ["identity", "amplification"]


@pytest.mark.parametrize("graph", list(GRAPHS_C))
@pytest.mark.parametrize("T,F", [(3, 5), (1, 130)])
@pytest.mark.parametrize("p", [0.5, 0.3])
def test_fused_scalar_width_with_dropout(graph, T, F, p):
    """F % 4 != 0: the keep factor of column c is byte c & 3 of quad c >> 2 (p = 0.5: one hash word, 0.3: two)."""
    L = GRAPHS_C[graph]()
    for by_pos in (True, False):
        check_fused(L, T, F, FUSED_AGGS, SC2, p, c_expect(L, 1), np.random.default_rng(F), by_pos=by_pos,
                    what="%s %dx%d p=%g by_pos=%d" % (graph, T, F, p, by_pos))


@pytest.mark.parametrize("graph", list(GRAPHS_C))
@pytest.mark.parametrize("demote", [dict(pad_uv=1), dict(pad_z=2), dict(u_shift=1)])
def test_fused_demoted_to_scalar_access(graph, demote):
    """F % 4 == 0 but lduv = 2 D + 1, ldz = D + 2, or a [U | V] base one float into a row: VEC 1, and the min / max blocks and args of the
    aligned run bit for bit."""
    L = GRAPHS_C[graph]()
    T, F = 2, 8
    ra, _ = check_fused(L, T, F, FUSED_AGGS, SC2, 0.5, c_expect(L, 4), np.random.default_rng(16), what=graph + " aligned")
    rd, _ = check_fused(L, T, F, FUSED_AGGS, SC2, 0.5, c_expect(L, 1), np.random.default_rng(16), what="%s %s" % (graph, demote), **demote)
    for k in (2, 3):
        assert np.array_equal(block_of(ra.out.numpy(), T, F, 4, 2, k), block_of(rd.out.numpy(), T, F, 4, 2, k))
    short = (L.deg > 0) & (L.deg < 256)
    assert np.array_equal(ra.amin[short], rd.amin[short]) and np.array_equal(ra.amax[short], rd.amax[short])
    assert np.array_equal(ra.gmsg[1], rd.gmsg[1]) and np.array_equal(ra.gmsg[2], rd.gmsg[2])


@pytest.mark.parametrize("graph", list(GRAPHS_C))
@pytest.mark.parametrize("Z", ["rows", None])
def test_fused_by_position_and_by_edge_id(graph, Z):
    """by_pos 0 and 1 index the Z rows and the gmsg rows by original id or by position: the same results either way; Z = None."""
    L = GRAPHS_C[graph]()
    T, F = 2, 8
    res = [check_fused(L, T, F, FUSED_AGGS, SC2, 0.5, c_expect(L, 4), np.random.default_rng(3), Z=Z, by_pos=bp,
                       what="%s Z=%s by_pos=%d" % (graph, Z, bp))[0] for bp in (True, False)]
    assert torch.equal(res[0].out, res[1].out)
    for a, b in zip(res[0].gmsg, res[1].gmsg):
        assert np.array_equal(a, b[L.perm])


@pytest.mark.parametrize("by_pos", [True, False])
@pytest.mark.parametrize("family", ["wave", "flat", "block"])
def test_fused_categorical_z_table(family, by_pos):
    """A 4-row Z table with a uint8 z_index in the wave kernel, the flat kernel (var in the list) and the block kernel; the 70-edge hub of
    the small graph takes the list pass behind the last two."""
    L = tiny_graph() if family == "wave" else small_graph()
    aggs = FUSED_AGGS + ["var"] if family == "flat" else FUSED_AGGS
    check_fused(L, 2, 8, aggs, SC2, 0.5, c_expect(L, 4, block=family == "block"), np.random.default_rng(4), Z="table", by_pos=by_pos,
                what="table %s by_pos=%d" % (family, by_pos))


@pytest.mark.parametrize("graph", list(GRAPHS_C))
def test_fused_row_pitched_operands(graph):
    """lduv = 2 D + 4, ldz = D + 4, ldsave = D + 4 (and ldg, ldgu): VEC 4 stays, the pitch columns are neither read nor written."""
    L = GRAPHS_C[graph]()
    check_fused(L, 2, 8, FUSED_AGGS, SC2, 0.5, c_expect(L, 4), np.random.default_rng(5), what=graph + " pitched", pad_uv=4, pad_z=4,
                pad_save=4, pad_g=4, pad_gu=4)


# ---- D. grid-stride loops --------------------------------------------------------------------------------------------------------------

def check_stride(L, aggs, expect, with_list=True, what=""):
    """Given messages at D = 4: out and the gradient strict, the max block, its saved args and its 0 / 1 pattern exact (vectorised
    oracle)."""
    T, F, K = 1, 4, len(aggs)
    rng = np.random.default_rng(L.N)
    inputs = quarters(rng, (L.E, 4))
    k = aggs.index("max")
    gouts = [rng.standard_normal((L.N, T, K * F)).astype(np.float32), R.onehot_gout(L.N, T, F, K, 1, k)]
    ref = R.reference(L, inputs, None, T, F, aggs, ["identity"], gouts)
    r = R.run(L, T, F, aggs, ["identity"], gouts, inputs=inputs, with_list=with_list, expect=expect)
    check_close(r.out, ref["out32"], None, None, what=what + " out")
    check_close(torch.from_numpy(r.gmsg[0]), ref["gmsg32"][0], None, None, what=what + " dL/dinputs")
    assert_empty_targets(L, r, ref, what)
    assert np.array_equal(block_of(r.out.numpy(), T, F, K, 1, k), block_of(ref["out32"], T, F, K, 1, k))
    assert np.array_equal(r.gmsg[1], ref["gmsg32"][1]), what + ": 0/1 gradient pattern of max"
    R.assert_saved_args(L, 4, r.amax, r.amax_side, R.arg_offsets_vectorised(L, inputs, "max"), what)


N_STRIDE = 2 * 8192 + 5               # the wave kernel's grid covers 4 * kMaxGrid = 8192 nodes per iteration


def test_wave_kernel_strides_behind_the_block_kernel():
    """long_nodes = None: the wave-per-node kernel scans all N row pointers in three iterations and takes ten 65..70-edge nodes placed
    at the start, around the first seam (8190..8195) and in the last nodes, so that its second and third iterations carry prefetched
    state that is used.  Nodes 8196..16379 are empty (no stretch of 8192 empties fits between hubs at these ids at this N)."""
    rng = np.random.default_rng(1)
    deg = rng.integers(1, 4, N_STRIDE)
    deg[8196:16380] = 0
    hubs = [3, 8190, 8191, 8192, 8193, 8195, 16380, 16384, 16387, 16388]
    deg[hubs] = [65, 66, 67, 68, 69, 70, 65, 66, 67, 70]
    L = R.Layout(deg, rng)
    check_stride(L, ["max"], dict(fwd="block", bwd="block", second="wave-long", vec=4), with_list=False, what="wave behind block")


def test_wave_kernel_strides_over_everything():
    """E > 16 N (17 edges per node): the wave kernel takes every node, three iterations."""
    L = R.Layout(np.full(N_STRIDE, 17), np.random.default_rng(2))
    check_stride(L, ["max"], dict(fwd="none", bwd="none", second="wave", vec=4), what="wave over everything")


def test_flat_kernel_strides_over_its_slots():
    """N = 16 * 8192 + 17: more node blocks than the flat kernels' 8192 workgroup slots (var in the list keeps the block kernel out)."""
    N = 16 * 8192 + 17
    L = R.Layout(np.random.default_rng(3).integers(0, 3, N), np.random.default_rng(4))
    check_stride(L, ["max", "var"], dict(fwd="flat", bwd="flat", second="list", vec=4), what="flat stride")
