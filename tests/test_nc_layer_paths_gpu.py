"""The MMA layer's PRODUCTION forward / backward (`functional.nc_local_layer`) against the CPU oracle over the dispatch matrix of
`mma_nc_fused_fwd` / `mma_nc_fused_bwd` (csrc/nc_fused.hip): the shared-gradient form (one (N,H) cotangent for all K masks,
selection state in the packed code rows `crow`), the node-level backward inside K2b's epilogue, dropout from the kernels' own hash,
P / Q / gP / gQ as column blocks of one (N, 2*K*H) buffer - at the widths (vector / scalar path, one / two column chunks, idle lanes
in a lane group, 1 .. 64 items per wavefront), mask counts (one K-slice, slices 4 + {1,2,3}), hub layouts (chunked hub targets AND
chunked hub sources) and launch forms (one launch / separate launches) the dispatch distinguishes.  Then the same with the
node-level backward as a launch of its own (`MMA_FUSE_NODE_BWD=0`: what `sharded.py` runs for every halo launch), and the per-row
maxima of [gP | gQ] the kernels merge by atomicMax, which the three-product dL/dx and weight-gradient GEMMs trust as scaling bounds.

Bar: `golden_util.check_close` with the float64 oracle as truth (no tolerance of this module's own).  Everything a case exists for
is ASSERTED on the plan, so that a change to the plan builder cannot quietly turn it into a copy of another case."""
import collections
import functools

import numpy as np
import pytest
import torch

from golden_util import check_close
from test_nc_gpu import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEL_KINDS = ("max", "min", "softmax", "softmin")          # the kinds that own a slot of the code row

# tag, N, H, aggregators, activation, avg degree, hub target degree, hub source degree, chunk, one_launch (the form K1 AND K2b take
# with graph.ONE_LAUNCH on: vector path, one column chunk, one K-slice, few hub elements - `small_plan`)
Case = collections.namedtuple("Case", "tag N H names act avg_deg hub hub_src chunk one_launch")
CASES = [
    # vector path, one column chunk, one K-slice.  These FIVE take the one-launch form, every one of them with hub slots in both plans
    # (the hub sums are done by the wavefront that draws the last ticket): h128_k4, h64_k2, h16_k8, h20_k3, h12_k1
    Case("h128_k4", 300, 128, ["sum", "mean", "max", "min"], "new_sigmoid", 4, 300, 200, 64, True),            # one item per wavefront
    Case("h64_k2", 257, 64, ["mean", "softmax"], "sigmoid", 4, 90, 70, 16, True),                              # 4 items per wavefront
    Case("h16_k8", 400, 16, ["sum", "mean", "max", "min", "softmax", "softmin", "mean3", "max2"], "new_sigmoid", 4, 100, 80, 32, True),
    Case("h20_k3", 200, 20, ["min2", "softmin", "sum"], "sigmoid", 4, 60, 50, 16, True),                       # 5 of 8 lanes of a group busy
    Case("h12_k1", 150, 12, ["max"], "new_sigmoid", 4, 70, 40, 16, True),                                      # 3 of 4 lanes busy
    # vector path, slices 4 + 3 / 4 + 2: k_base > 0, first_pass = 0, gx and the hub partials accumulate over two launches
    Case("h64_k7", 250, 64, ["max", "mean", "softmax", "min", "softmin", "min2", "max3"], "new_sigmoid", 4, 120, 90, 32, False),
    Case("h16_k6", 300, 16, ["sum", "softmin", "max", "mean", "softmax", "min"], "sigmoid", 4, 80, 60, 16, False),
    # vector path, two column chunks (gridDim.y = 2), slices 4 + 1
    Case("h260_k5", 80, 260, ["max", "softmax", "mean", "min", "softmin"], "new_sigmoid", 3, 70, 50, 16, False),
    # scalar path (H % 4 != 0: bytes of a code word stay unwritten), two chunks, slices 4 + 2
    Case("h75_k6", 120, 75, ["softmin", "mean", "max", "sum", "min", "softmax"], "sigmoid", 4, 90, 60, 32, False),
    # scalar path, 8 items per wavefront, slices 4 + 3
    Case("h6_k7", 200, 6, ["sum", "min", "mean", "max", "max2", "softmin", "min3"], "new_sigmoid", 4, 60, 50, 16, False),
    # scalar path, no mask needs a code row: crow is the 4-float header alone
    Case("h3_k2", 150, 3, ["sum", "mean"], "sigmoid", 4, 50, 40, 16, False),
    # H = 1: 64 items per wavefront, lane groups of ONE lane
    Case("h1_k4", 200, 1, ["mean", "max", "softmax", "min"], "new_sigmoid", 4, 60, 50, 16, False),
]
BY_TAG = {c.tag: c for c in CASES}
P_ASKED = [0.0, 0.5, 0.3]        # none; a multiple of 1/256 (the one-word HASH kernels); not one (the HASH16 kernels)
SEED = 0x0123456789ABCDEF


def slices_of(K):
    """K-slices the launchers issue (`next_slice`): 8 | 4 + {1,2,3} | {1,2,3,4}."""
    out, k0 = [], 0
    while k0 < K:
        ks = 8 if K - k0 >= 8 else (4 if K - k0 >= 4 else K - k0)
        out.append((k0, ks))
        k0 += ks
    return out


def geometry(H):
    """(vec, lpr_log, chunks, items per wavefront) as `geometry()` in nc_shared.h picks them for the buffers of the layer."""
    vec = 4 if H % 4 == 0 else 1
    per_row = -(-H // vec)
    lpr_log = min((per_row - 1).bit_length(), 6)
    return vec, lpr_log, -(-per_row // (1 << lpr_log)), 64 >> lpr_log


def takes_one_launch(graph, H, K, backward):
    """`small_plan` of nc_fused.hip restated on the plan (hash / no dropout, a sync counter given)."""
    vec, lpr_log, chunks, ipw = geometry(H)
    items, n_wave, hubs = (graph.t_items, graph.t_n_wave_items, graph.t_hubs) if backward else (graph.items, graph.n_wave_items, graph.hubs)
    n_items, n_hubs = items.shape[0], hubs.shape[0]
    if ipw == 1:
        n_wave = n_items
    if vec != 4 or chunks != 1 or K not in (1, 2, 3, 4, 8) or n_hubs * -(-H // 4) * ((K + 1) if backward else 1) > 4096:
        return False
    return not (n_hubs == 0 and (n_wave == 0 or n_items == n_wave))


# ---- what the matrix has to contain (checked when the module is collected, GPU or not) ---------------------------------------------
def _matrix_is_complete():
    from oracle.nc_oracle import AGGREGATORS
    kinds = lambda names: [AGGREGATORS[n][0] for n in names]
    assert {c.H for c in CASES} >= {128, 64, 16, 20, 12, 260, 75, 6, 3, 1}
    assert {len(c.names) for c in CASES} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {k for c in CASES for k in kinds(c.names)} == {"sum", "mean", "max", "min", "softmax", "softmin"}
    assert {c.act for c in CASES} == {"sigmoid", "new_sigmoid"}
    sliced = [c for c in CASES if len(slices_of(len(c.names))) == 2]
    assert {len(c.names) for c in sliced} == {5, 6, 7}
    for s in (0, 1):        # every code-row kind on both sides of a slice boundary
        seen = {k for c in sliced for k in kinds(c.names)[slices_of(len(c.names))[s][0]:][:slices_of(len(c.names))[s][1]]}
        assert seen >= set(SEL_KINDS), (s, seen)
    assert any(not set(kinds(c.names)) & set(SEL_KINDS) for c in CASES)                 # a code row that is the header alone
    assert sum(c.one_launch and c.hub > c.chunk and c.hub_src > c.chunk for c in CASES) >= 3
    assert {geometry(c.H)[:3] + (len(slices_of(len(c.names))),) for c in CASES} >= {
        (4, 5, 1, 1), (4, 4, 1, 1), (4, 2, 1, 1), (4, 3, 1, 1), (4, 4, 1, 2), (4, 2, 1, 2), (4, 6, 2, 2), (1, 6, 2, 2), (1, 3, 1, 2),
        (1, 2, 1, 1), (1, 0, 1, 1)}


_matrix_is_complete()


# ---- the problems (CPU) and their oracle values ------------------------------------------------------------------------------------
def with_hub_sources(rng, rowptr, col, N, hub_src):
    """`random_graph` makes hub TARGETS (long rows).  Point `hub_src` random edges at node N-3 and hub_src // 2 + 1 at node N-4, so that
    the transposed plan has hubs as well, and detach node 0 (degree 0 already) from every row: a node without any edge in either plan.  Node 2 (degree 1) is no source either."""
    col = col.copy()
    E = len(col)
    for node, n in ((N - 3, hub_src), (N - 4, hub_src // 2 + 1)):
        if n:
            col[rng.choice(E, size=n, replace=False)] = node
    col[col == 0] = N // 2
    col[col == 2] = N // 2 + 1          # node 2 (degree 1): no outgoing edge
    return col


Problem = collections.namedtuple("Problem", "case p_asked thr p seed rowptr col E x Ws wcat cot keep kinds acts")


@functools.lru_cache(maxsize=None)
def problem(tag, p_asked):
    from mma_amd import functional as Fn
    from oracle import nc_oracle as O
    from oracle.dropout_rng import keep_mask16, threshold16
    c = BY_TAG[tag]
    N, H, K = c.N, c.H, len(c.names)
    rng = np.random.default_rng(77 + N + 1000 * H)
    rowptr, col = random_graph(rng, N, c.avg_deg, c.hub)
    col = with_hub_sources(rng, rowptr, col, N, c.hub_src)
    E = int(rowptr[-1])
    x = torch.from_numpy(np.maximum(rng.standard_normal((N, H)), 0).astype(np.float32))
    Ws = [torch.from_numpy(((rng.random((2 * H, H)) * 2 - 1) / np.sqrt(H)).astype(np.float32)) for _ in c.names]
    wcat = torch.cat([W[:H] for W in Ws] + [W[H:] for W in Ws], 1).contiguous()          # functional.mask_weights' layout
    cot = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
    thr = threshold16(p_asked)
    seed = SEED
    keep = keep_mask16(seed, thr, K, E, H) if thr else None
    kinds = tuple(Fn.KIND[O.AGGREGATORS[n][0]] for n in c.names)
    acts = tuple(Fn.ACT_RAW if O.uses_raw_logits(n, c.act) else Fn.ACT_SIGMOID for n in c.names)
    return Problem(c, p_asked, thr, thr / 65536.0, seed, rowptr, col, E, x, Ws, wcat, cot, keep, kinds, acts)


@functools.lru_cache(maxsize=None)
def oracle(tag, p_asked, dtype):
    """(out, dL/dx, dL/dwcat) of sum_k aggregate_k by the CPU oracle, fed the keep bits of the kernels' hash; all finite."""
    from oracle import nc_oracle as O
    pb = problem(tag, p_asked)
    c, H = pb.case, pb.case.H
    xo = pb.x.to(dtype, copy=True).requires_grad_(True)          # copies: the problem's own tensors stay leaves without a gradient
    Wo = [W.to(dtype, copy=True).requires_grad_(True) for W in pb.Ws]
    out = sum(O.aggregate(n, xo, Wo[k], pb.rowptr, pb.col, c.act, pb.p, None if pb.keep is None else pb.keep[k])
              for k, n in enumerate(c.names))
    g = torch.autograd.grad((out * pb.cot.to(dtype)).sum(), [xo] + Wo)
    gw = torch.cat([gk[:H] for gk in g[1:]] + [gk[H:] for gk in g[1:]], 1)
    res = (out.detach().numpy(), g[0].numpy(), gw.numpy())
    # the softmax NaN bands are pinned in test_nc_gpu.py; here every value has to be a number, in fp32 as well
    assert all(np.isfinite(r).all() for r in res), "oracle (%s) not finite for %s p=%g" % (dtype, tag, p_asked)
    return res


def build_graph(pb):
    """The plan with everything the case exists for asserted on it."""
    import mma_amd
    c = pb.case
    H, K = c.H, len(c.names)
    graph = mma_amd.NCGraph(pb.rowptr, pb.col, DEV, chunk=c.chunk, group_below=4, t_group_below=4)
    deg, tdeg = np.diff(pb.rowptr), np.bincount(pb.col, minlength=c.N)
    assert (deg == 0).sum() >= 2 and (deg == 1).sum() >= 2 and deg[0] == 0 and tdeg[0] == 0          # degree 0 / 1; node 0 in no edge
    assert graph.n_slots > 0 and graph.t_n_slots > 0                                                 # hub chunks in BOTH plans
    assert graph.hubs.shape[0] >= 2 and graph.t_hubs.shape[0] >= 2
    assert 0 < graph.n_wave_items < graph.items.shape[0] and 0 < graph.t_n_wave_items < graph.t_items.shape[0]
    assert (H % 4 == 0) == (geometry(H)[0] == 4)
    assert takes_one_launch(graph, H, K, False) == c.one_launch and takes_one_launch(graph, H, K, True) == c.one_launch
    return graph


def run_layer(pb, graph):
    from mma_amd import functional as Fn
    xg, wg = pb.x.to(DEV).requires_grad_(True), pb.wcat.to(DEV).requires_grad_(True)
    out = Fn.nc_local_layer(xg, wg, None, graph, pb.kinds, pb.acts, Fn.DropoutSpec(pb.p_asked, seed=pb.seed))
    gx, gw = torch.autograd.grad((out * pb.cot.to(DEV)).sum(), [xg, wg])
    return out.detach(), gx, gw


def check_against_oracle(got, tag, p_asked, what):
    want, truth = oracle(tag, p_asked, torch.float32), oracle(tag, p_asked, torch.float64)
    for name, g, w, t in zip(("out", "gx", "gwcat"), got, want, truth):
        check_close(g, w, None, None, what="%s %s/%s" % (what, tag, name), signed_sum=True, truth=t)


def sync_is_zero(graph):
    return getattr(graph, "_sync", None) is None or int(graph._sync.abs().sum()) == 0


# ---- 1. the layer over the dispatch matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_asked", P_ASKED, ids=lambda p: "p%g" % p)
@pytest.mark.parametrize("tag", [c.tag for c in CASES])
def test_layer_against_the_oracle(tag, p_asked, monkeypatch):
    """out, dL/dx, dL/dwcat of `nc_local_layer` (shared gradient, code rows, epilogue, hash dropout, [P|Q] / [gP|gQ] in one buffer)
    against the float64 oracle, as one launch and as separate launches.  Where `small_plan` refuses the one-launch form the switch
    must change nothing; where it takes it the hub sums move into the item kernel but keep their order: bit equality either way.
    A second call gives the same bits, the ticket counters are back at zero after every call, and the forward equals
    `nc_fused_aggregate(reduce_k=True)` on the two column blocks of the same [P|Q] buffer."""
    from mma_amd import dense, functional as Fn, graph as G
    pb = problem(tag, p_asked)
    c = pb.case
    N, H, K = c.N, c.H, len(c.names)
    assert Fn.SHARED_GRAD_BWD and Fn.FUSE_NODE_BWD, "this test is about the default (production) form"
    spec = Fn.DropoutSpec(p_asked, seed=pb.seed)
    assert spec.thr == pb.thr and spec.mode == (Fn.DROP_HASH if p_asked else Fn.DROP_NONE) and (pb.thr % 256 == 0) == (p_asked != 0.3)
    assert len(slices_of(K)) == (2 if K in (5, 6, 7) else 1)
    assert Fn.crow_floats(H, pb.kinds) == (4 + sum(n.rstrip("234") in SEL_KINDS for n in c.names) * -(-H // 4) + 3) // 4 * 4
    graph = build_graph(pb)
    res = {}
    for one in (True, False):
        monkeypatch.setattr(G, "ONE_LAUNCH", one)
        assert (graph.sync(0) is not None) == one and (graph.sync(1) is not None) == one
        got = run_layer(pb, graph)
        assert sync_is_zero(graph)
        check_against_oracle(got, tag, p_asked, "one launch" if one else "separate launches")
        again = run_layer(pb, graph)
        assert sync_is_zero(graph)
        for a, b in zip(got, again):
            assert torch.equal(a, b), "a second identical call differs"
        # the unshared entry point on views of one buffer (row pitch 2*K*H): the same forward kernel on the same operands
        PQ = torch.empty((N, 2 * K * H), device=DEV, dtype=torch.float32)
        xg = pb.x.to(DEV)
        dense.mm_into(xg, pb.wcat.to(DEV), PQ)
        agg = Fn.nc_fused_aggregate(xg.requires_grad_(True), PQ[:, :K * H], PQ[:, K * H:], graph, pb.kinds, pb.acts, spec, reduce_k=True)
        assert sync_is_zero(graph)
        assert torch.equal(agg.detach(), got[0]), "nc_local_layer's forward differs from nc_fused_aggregate(reduce_k=True)"
        res[one] = got
    assert graph._sync is not None
    for name, a, b in zip(("out", "gx", "gwcat"), res[True], res[False]):
        assert torch.equal(a, b), "%s: ONE_LAUNCH on / off differ in %s" % (tag, name)


# ---- 2. the node-level backward as a launch of its own -------------------------------------------------------------------------------
# one case per (path, column chunks, K-slices) class, all with hubs in both plans
UNFUSED = ["h128_k4", "h64_k7", "h260_k5", "h75_k6", "h6_k7", "h1_k4", "h3_k2"]


@pytest.mark.parametrize("p_asked", [0.5, 0.3], ids=lambda p: "p%g" % p)
@pytest.mark.parametrize("tag", UNFUSED)
def test_unfused_node_backward_against_the_oracle(tag, p_asked, monkeypatch):
    """`functional.FUSE_NODE_BWD = False` (MMA_FUSE_NODE_BWD=0): K2a (`nc_bwd_node_kernel`, reading the code rows, gP a column block
    of [gP|gQ]) as a launch of its own, then K2b without the epilogue - the form `sharded.py` runs for every halo launch - against
    the float64 oracle by the same bar as the fused form.  The two forms restate the same formulas (`nc_bwd_node_kernel` /
    `nc_bwd_epilogue`) but assemble dL/dx differently, so this side needs the reference of its own; how they compare bit for bit
    is asserted as measured on the MI355X (`compare_fused_with_unfused`)."""
    from mma_amd import functional as Fn, graph as G
    pb = problem(tag, p_asked)
    graph = build_graph(pb)
    res = {}
    for one in (True, False):
        monkeypatch.setattr(G, "ONE_LAUNCH", one)
        monkeypatch.setattr(Fn, "FUSE_NODE_BWD", False)
        got = run_layer(pb, graph)
        assert sync_is_zero(graph)
        check_against_oracle(got, tag, p_asked, "unfused K2a, " + ("one launch" if one else "separate launches"))
        res[one] = got
        monkeypatch.setattr(Fn, "FUSE_NODE_BWD", True)
        fused = run_layer(pb, graph)
        compare_fused_with_unfused(tag, fused, got)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def compare_fused_with_unfused(tag, fused, unfused):
    """Measured on the MI355X over UNFUSED x {0.5, 0.3} x both launch forms: out and dL/dwcat are bit-equal in every case (the forward
    is the same launch, and gP / gQ come out of the same expressions in both forms), and so is dL/dx with one K-slice (direct term +
    edge sum, in that order, either way).  With two K-slices dL/dx is NOT: fused it is ((d1 + e1) + d2) + e2, unfused
    ((d1 + d2) + e1) + e2 (d: direct term, e: edge sum of a slice) - largest difference seen 3.8e-6 absolute (h64_k7, h75_k6),
    inside the strict 1e-5 + 1e-5|ref| bar, i.e. 0 in units of check_close's noise multiple.  Only the oracle bar holds there."""
    one_slice = len(slices_of(len(BY_TAG[tag].names))) == 1
    for name, a, b in zip(("out", "gx", "gwcat"), fused, unfused):
        if name != "gx" or one_slice:
            assert torch.equal(a, b), "%s: %s differs between the fused and the unfused node-level backward" % (tag, name)


# ---- 3. the row maxima of [gP | gQ] ---------------------------------------------------------------------------------------------------
ALL_DROPPED = Case("h4_k1_dropped", 200, 4, ["sum"], "sigmoid", 4, 60, 50, 16, True)
BY_TAG[ALL_DROPPED.tag] = ALL_DROPPED
ROW_MAX = [("h128_k4", 0.5), ("h16_k8", 0.3), ("h64_k7", 0.3), ("h260_k5", 0.5), ("h75_k6", 0.3), ("h6_k7", 0.5), ("h3_k2", 0.0),
           ("h1_k4", 0.3), ("h20_k3", 0.0), (ALL_DROPPED.tag, 0.9373)]


@pytest.mark.parametrize("tag,p_asked", ROW_MAX, ids=["%s_p%g" % tp for tp in ROW_MAX])
def test_row_maxima_equal_the_rows_they_stand_for(tag, p_asked, monkeypatch):
    """`row_max[i]` = max |[gP|gQ][i, :]| as K2a or the epilogue, the K2b items and the hub finalize leave it (atomicMax over the
    values they store): in production it only exists from 65536 rows on, where the three-product dL/dx and weight-gradient GEMMs
    scale every row by it - too small a value overflows an fp16 piece.  Here the launch helpers are called directly on a few
    hundred rows, fused and unfused, as one launch and as separate launches, with sliced K (two launches merge into one maximum),
    hub sources (finalize), the scalar path, a node in no edge at all and a row whose every mask element is dropped (all-zero row:
    the maximum has to stay exactly 0, that is what the GEMMs take as "skip the row").  The maxima are taken over exactly the
    stored values, so EQUALITY is the contract, not a bound."""
    from mma_amd import functional as Fn, graph as G
    pb = problem(tag, p_asked)
    c = pb.case
    N, H, K = c.N, c.H, len(c.names)
    KH = K * H
    graph = build_graph(pb)
    x, wcat, g = pb.x.to(DEV), pb.wcat.to(DEV), pb.cot.to(DEV)
    PQ = x @ wcat
    P, Q = PQ[:, :KH], PQ[:, KH:]
    drop = Fn.DropoutSpec(p_asked, seed=pb.seed)
    if tag == ALL_DROPPED.tag:
        # node 2: one incoming edge whose H elements are all dropped (checked on the CPU for SEED), no outgoing edge
        assert pb.rowptr[3] - pb.rowptr[2] == 1 and not pb.keep[:, pb.rowptr[2], :].any() and not (pb.col == 2).any()
    res = []
    for one in (True, False):
        monkeypatch.setattr(G, "ONE_LAUNCH", one)
        for fused in (True, False):
            msum, T, sel, crow = Fn.nc_fwd_launch(x, P, Q, graph, pb.kinds, pb.acts, drop, True, True)
            assert sel is None and crow is not None and tuple(crow.shape) == (N, Fn.crow_floats(H, pb.kinds))
            gPQ = torch.full((N, 2 * KH), float("nan"), device=DEV)
            gx = torch.full((N, H), float("nan"), device=DEV)
            rm = torch.zeros((N,), device=DEV)
            partial = torch.empty((graph.t_n_slots, (K + 1) * H), device=DEV)
            if fused:
                Fn.nc_bwd_edges_launch(x, P, Q, None, g, crow, None, graph, pb.kinds, pb.acts, drop, gPQ[:, KH:], gx, partial,
                                       row_max=rm, T=T, gP=gPQ[:, :KH])
            else:
                gs, gP, gxs = Fn.nc_bwd_node_launch(g, True, None, crow, T, graph, pb.kinds, H, True, gP=gPQ[:, :KH], row_max=rm)
                assert gs is None and gP.data_ptr() == gPQ.data_ptr()
                Fn.nc_bwd_edges_launch(x, P, Q, None, g, crow, gxs, graph, pb.kinds, pb.acts, drop, gPQ[:, KH:], gx, partial, row_max=rm)
            assert sync_is_zero(graph)
            assert torch.isfinite(gPQ).all() and torch.isfinite(gx).all(), "an element of [gP|gQ] or gx was not written"
            want = gPQ.abs().amax(1)
            bad = torch.nonzero(rm != want).flatten()
            assert bad.numel() == 0, "%s one=%s fused=%s: row_max != max|row| on %d rows, first %d: %r vs %r" % (
                tag, one, fused, bad.numel(), int(bad[0]), float(rm[bad[0]]), float(want[bad[0]]))
            assert float(rm[0]) == 0.0 and not gPQ[0].any()                 # node 0: in no edge of either plan
            assert int((rm == 0).sum()) < N // 2 and float(rm.max()) > 0
            if tag == ALL_DROPPED.tag:
                assert float(rm[2]) == 0.0 and not gPQ[2].any()
            res.append((gPQ, rm, fused))
    for gPQ, rm, fused in res[1:]:      # [gP|gQ] itself does not depend on the form (gx does: see the unfused test)
        assert torch.equal(gPQ, res[0][0]) and torch.equal(rm, res[0][1])
