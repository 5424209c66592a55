"""GPU tests of the HALO form of the node-classification kernels (include/mma_amd.h: K1 / K2a / K2b of csrc/nc_fused.hip, K1s / K2s of
csrc/nc_moments.hip, and their bf16-table `_h` twins), in one process and against the float64 oracle: x and Q have n_src = S >= N rows of
which rows [N, S) are sources only, the backward runs over S source rows with n_targets = N, and the dropout hash is keyed with global
edge positions (drop_edge_base).  Everything goes through the public functions of mma_amd.functional on an NCGraph(..., n_src=S,
edge_base=...) - no layer, no process group.

A halo problem IS an ordinary S-node graph in which rows >= N take no in-edge and a zero cotangent (nc_layer_util.embed), so the plain
torch oracles of the no-halo files state it unchanged: their m[:N], their gx on all S rows and their mask-weight gradients are the values
to meet.  float64 on the CPU is the truth, the same statement in float32 the reference value, and the bar is the project's own, unchanged
(golden_util.check_close with truth), over all rows and elements.

The graph (nc_layer_util.halo_graph) is the smallest on which the halo form takes every path it has: a hub target over own and halo
sources, the boundary in-degrees from halo sources alone, an OWN hub source and HALO hub sources (the `node < n_targets` of K2b's item
path and of its hub sums), the boundary out-degrees on halo sources, and sources - own ones and a halo one - with no out-edge, whose rows
of gQ / gx nothing but a store of zero fills.  `test_the_plan_reaches_the_paths` asserts all of that on the plan.

Inputs: the fp32 cases draw x and the weights as the no-halo test of the same kernel does (test_nc_gpu.py, nc_layer_util.std_inputs); the
bf16 cases use the grids of test_nc_bf16_gpu.py (x on 2^-5, weights on 2^-9), on which P and Q are exact in every arithmetic, so that the
three sides round the same tables (asserted bit for bit)."""
import functools
import math

import numpy as np
import pytest
import torch

from golden_util import check_close
from nc_layer_util import BF16, BOUNDARY_DEGREES, DEV, csr_of, degenerate_targets, embed, halo_graph, std_inputs
from nc_layer_util import oracle_with_grads as std_oracle_with_grads
from test_nc_bf16_gpu import EIGHT, FIVE
from test_nc_bf16_gpu import oracle_with_grads as fused_oracle_with_grads
from oracle import nc_oracle as O
from oracle.dropout_rng import keep_mask16, threshold16

pytestmark = pytest.mark.gpu
F32 = torch.float32
ADD, S = halo_graph()
N = len(ADD)
FULL = embed(ADD, S)
DEG, COL = csr_of(ADD)
ROWPTR = np.concatenate([[0], np.cumsum(DEG)]).astype(np.int64)
E = int(ROWPTR[-1])
OUT_DEG = np.bincount(COL, minlength=S)
NO_OUT_OWN = np.nonzero(OUT_DEG[:N] == 0)[0]
NO_OUT = np.nonzero(OUT_DEG == 0)[0]
SEED = 0x1234567890ABCDEF
BASES = {"base12345": 12345, "baseMax": 2 ** 32 - 1 - E}          # the second: the largest base make_drop (nc_shared.h) accepts
SQRT_EPS = np.float32(math.sqrt(1e-5))
NAMES = {"K5": FIVE, "K8": EIGHT}
tname = lambda bf16: "bf16" if bf16 else "fp32"


@functools.lru_cache(maxsize=None)
def plan(chunk, edge_base=0, device=DEV):
    import mma_amd
    return mma_amd.NCGraph(ROWPTR, COL, device, n_src=S, chunk=chunk, group_below=8, t_group_below=8, edge_base=edge_base)


# ---- the graph and its plans (no kernel runs) --------------------------------------------------------------------------------------
def test_the_plan_reaches_the_paths():
    assert (N, S, E) == (150, 300, 1381)
    assert DEG[:10].tolist() == [200] + BOUNDARY_DEGREES and OUT_DEG[290:].tolist() == [100] + BOUNDARY_DEGREES
    assert all(s >= N for t in range(1, 10) for s in ADD[t])                   # targets 1..9: halo sources only
    assert min(ADD[0]) < N <= max(ADD[0])                                      # the hub target: own and halo sources
    assert len(NO_OUT_OWN) == 21 and NO_OUT[NO_OUT >= N].tolist() == [291]
    assert degenerate_targets(ADD) == [1, 2] and len(degenerate_targets(ADD)) <= 0.05 * N
    assert FULL[:N] == ADD and FULL[N:] == [[]] * (S - N)
    g = plan(32, device="cpu")
    assert (g.N, g.n_src, g.E) == (N, S, E) and g.sync(0) is None and g.sync(1) is None
    assert g.hubs[:, 0].tolist() == [0, 7, 8, 9] and g.n_slots == 14
    assert g.t_hubs[:, 0].tolist() == [10, 290, 297, 298, 299] and g.t_n_slots == 15          # an own hub source and halo hub sources
    (h_items, h_wave, h_hubs), (o_items, o_wave, o_hubs) = g.t_parts
    assert h_items.shape[0] == 157 and h_hubs[:, 0].tolist() == [290, 297, 298, 299] and bool((h_items[:, 0] >= N).all())
    assert o_items.shape[0] == 153 and o_hubs[:, 0].tolist() == [10] and bool((o_items[:, 0] < N).all())
    assert 0 < h_wave < h_items.shape[0] and 0 < o_wave < o_items.shape[0]                    # wavefront items and grouped items in both
    assert 0 < g.n_wave_items < g.items.shape[0]
    w = plan(512, device="cpu")
    assert w.n_slots == 0 and w.t_n_slots == 0
    assert plan(32, BASES["baseMax"], "cpu").edge_base + E == 2 ** 32 - 1


# ---- the problems (CPU) and their oracle values ------------------------------------------------------------------------------------
class Fused:
    """x (S,H), K mask weights (2H,H), cotangents (N,H) and (K,N,H) of one fused case."""

    def __init__(self, H, bf16, activation, names):
        from mma_amd import functional as Fn
        self.H, self.bf16, self.activation, self.names, self.K = H, bf16, activation, list(names), len(names)
        rng = np.random.default_rng(1234 + S + H)
        u = lambda: (rng.random((2 * H, H)) * 2 - 1) / np.sqrt(H)
        if bf16:      # the grids of test_nc_bf16_gpu.py
            self.x = torch.from_numpy((rng.integers(-32, 33, (S, H)) / 32.0).astype(np.float32))
            self.Ws = [torch.from_numpy((np.round(u() * 512.0) / 512.0).astype(np.float32)) for _ in names]
        else:         # as test_nc_gpu.py: test_random_graph_vs_oracle
            self.x = torch.from_numpy(np.maximum(rng.standard_normal((S, H)), 0).astype(np.float32))
            self.Ws = [torch.from_numpy(u().astype(np.float32)) for _ in names]
        self.cot = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
        self.cot_k = torch.from_numpy(rng.standard_normal((self.K, N, H)).astype(np.float32))
        self.kinds = [Fn.KIND[O.AGGREGATORS[n][0]] for n in names]
        self.acts = [Fn.ACT_RAW if O.uses_raw_logits(n, activation) else Fn.ACT_SIGMOID for n in names]
        self.table_dtype = BF16 if bf16 else F32
        self.tag = "halo/fused/H%d/%s/%s/K%d" % (H, tname(bf16), activation, self.K)


@functools.lru_cache(maxsize=None)
def fused_problem(H, bf16, activation, names_key):
    return Fused(H, bf16, activation, NAMES[names_key])


def keep_bits(K, H, p_asked, edge_base):
    """The keep mask (K,E,H) of the kernels' hash at GLOBAL edge positions, and the probability they apply."""
    thr = threshold16(p_asked)
    if not thr:
        return None, 0.0
    return keep_mask16(SEED, thr, K, E, H, edge_ids=edge_base + np.arange(E)), thr / 65536.0


def pad(t):
    """A cotangent (..., N, H) with zero rows for the halo sources, for the oracle only."""
    return torch.cat([t, torch.zeros(t.shape[:-2] + (S - N, t.shape[-1]), dtype=t.dtype)], -2)


@functools.lru_cache(maxsize=None)
def fused_oracles(H, bf16, activation, names_key, p_asked=0.0, edge_base=0):
    """(float32 reference, float64 truth) of one fused case, once: m and msum on the N targets, gx on all S rows."""
    pb = fused_problem(H, bf16, activation, names_key)
    keep, p = keep_bits(pb.K, H, p_asked, edge_base)
    keeps = None if keep is None else torch.from_numpy(keep)
    out = []
    for dt in (F32, torch.float64):
        r = fused_oracle_with_grads(pb.x, pb.Ws, pb.names, FULL, activation, pad(pb.cot), pad(pb.cot_k), keeps, p, dt, pb.table_dtype)
        r["m"], r["msum"] = r["m"][:, :N], r["msum"][:N]
        assert all(np.isfinite(a).all() for v in r.values() for a in (v if isinstance(v, list) else [v])), "oracle (%s) not finite for %s" % (dt, pb.tag)
        out.append(r)
    return tuple(out)


class Std:
    def __init__(self, H, bf16, activation):
        from mma_amd import functional as Fn
        self.H, self.bf16, self.activation = H, bf16, activation
        x, cot = std_inputs(FULL, H, x_grid=bf16)          # x (S,H); the cotangent is zero wherever the exact variance is zero ...
        assert not cot[N:].any() and len(degenerate_targets(ADD)) <= 0.05 * N         # ... so on every halo row, and on 2 of 150 targets
        assert degenerate_targets(FULL)[:2] == degenerate_targets(ADD)
        self.x, self.cot = x, cot[:N].contiguous()
        w = (np.random.default_rng(40 + H).random((2 * H, H)) * 2 - 1) / np.sqrt(H)          # U(+-1/sqrt(H)), as the layer draws mask_std
        self.W = torch.from_numpy((np.round(w * 512.0) / 512.0 if bf16 else w).astype(np.float32))
        self.act = Fn.ACT_RAW if activation == "new_sigmoid" else Fn.ACT_SIGMOID
        self.table_dtype = BF16 if bf16 else F32
        self.tag = "halo/std/H%d/%s/%s" % (H, tname(bf16), activation)


@functools.lru_cache(maxsize=None)
def std_problem(H, bf16, activation):
    return Std(H, bf16, activation)


@functools.lru_cache(maxsize=None)
def std_oracles(H, bf16, activation, p_asked=0.0, edge_base=0):
    """(float32 reference, float64 truth) of one std case: (m on the N targets, gx on all S rows, gmask_std)."""
    pb = std_problem(H, bf16, activation)
    keep, p = keep_bits(1, H, p_asked, edge_base)
    keep = None if keep is None else torch.from_numpy(keep[0])
    out = []
    for dt in (F32, torch.float64):
        m, gx, gw = std_oracle_with_grads(pb.x, pb.W, FULL, activation, pad(pb.cot), keep, p, dt, pb.table_dtype)
        out.append((m[:N], gx, gw))
    return tuple(out)


def compare_one(got, want, truth, what):
    g = got.detach().cpu().numpy().astype(np.float64)
    print("%s: max |got - fp64| %.3g, max |fp32 ref - fp64| %.3g" % (what, np.nanmax(np.abs(g - truth)), np.nanmax(np.abs(want.astype(np.float64) - truth))))
    check_close(got, want, None, None, what=what, signed_sum=True, truth=truth)


def compare_fused(got, want, truth, names, what):
    for part, g in got.items():
        if isinstance(g, (list, tuple)):
            for k, n in enumerate(names):
                compare_one(g[k], want[part][k], truth[part][k], "%s/%s[%s]" % (what, part, n))
        elif part == "m":
            for k, n in enumerate(names):
                compare_one(g[k], want["m"][k], truth["m"][k], "%s/m[%s]" % (what, n))
        else:
            compare_one(g, want[part], truth[part], "%s/%s" % (what, part))


# ---- the runs (GPU) -----------------------------------------------------------------------------------------------------------------
def tables_are_the_oracles(x, Wtop, Wbot, P, Q):
    """On the grids P and Q are exact, so the bf16 tables the kernels gather are the oracle's rounded tables, bit for bit."""
    from mma_amd import functional as Fn
    for got, want, w64 in ((P, x[:N] @ Wtop, x[:N].double() @ Wtop.double()), (Q, x @ Wbot, x.double() @ Wbot.double())):
        assert torch.equal(want.double(), w64)
        assert torch.equal(Fn.rows_to_bf16(got.detach()).cpu().view(torch.int16), want.to(BF16).view(torch.int16))


def run_fused(pb, graph, drop=None, reduce_k=True):
    """nc_fused_aggregate with P / Q by torch, so that autograd carries gP / gQ to x and the mask weights: what fused_oracles returns,
    under the names of the path (msum, gx, gmask with reduce_k; m, gx_k, gmask_k without)."""
    from mma_amd import functional as Fn
    H = pb.H
    xg = pb.x.to(DEV).requires_grad_(True)
    Wg = [w.to(DEV).requires_grad_(True) for w in pb.Ws]
    P = xg[:N] @ torch.cat([w[:H] for w in Wg], 1)
    Q = xg @ torch.cat([w[H:] for w in Wg], 1)
    if pb.bf16:
        tables_are_the_oracles(pb.x, torch.cat([w[:H] for w in pb.Ws], 1), torch.cat([w[H:] for w in pb.Ws], 1), P, Q)
    out = Fn.nc_fused_aggregate(xg, P, Q, graph, pb.kinds, pb.acts, drop, reduce_k=reduce_k, logit_dtype=BF16 if pb.bf16 else None)
    assert out.shape == ((N, H) if reduce_k else (pb.K, N, H))
    g = torch.autograd.grad((out * (pb.cot if reduce_k else pb.cot_k).to(DEV)).sum(), [xg] + Wg)
    torch.cuda.synchronize()
    assert g[0].shape == (S, H)
    if reduce_k:
        return {"msum": out.detach(), "gx": g[0], "gmask": list(g[1:])}
    return {"m": out.detach(), "gx_k": g[0], "gmask_k": list(g[1:])}


def run_std(pb, graph, drop=None):
    """(m, gx, gmask_std) of nc_std_aggregate, P / Q by torch."""
    from mma_amd import functional as Fn
    H = pb.H
    xg = pb.x.to(DEV).requires_grad_(True)
    Wg = pb.W.to(DEV).requires_grad_(True)
    P, Q = xg[:N] @ Wg[:H], xg @ Wg[H:]
    if pb.bf16:
        tables_are_the_oracles(pb.x, pb.W[:H], pb.W[H:], P, Q)
    m = Fn.nc_std_aggregate(xg, P, Q, graph, pb.act, drop, logit_dtype=BF16 if pb.bf16 else None)
    assert m.shape == (N, H)
    gx, gw = torch.autograd.grad((m * pb.cot.to(DEV)).sum(), [xg, Wg])
    torch.cuda.synchronize()
    assert gx.shape == (S, H)
    return m.detach(), gx, gw


# ---- 1. the fused aggregators against the oracle ---------------------------------------------------------------------------------------
# shared: reduce_k, the shared-gradient form, K2a in K2b's epilogue (production); unfused: the same with K2a as a launch of its own;
# unshared: sel + gs - per mask (reduce_k=False) and, with SHARED_GRAD_BWD off, for the one shared cotangent.
# The raw logits of new_sigmoid come with the bf16 cases only: with the half-normal x of the fp32 draw the 200-edge hub target pushes
# softmax's exp(s) past the fp32 range (the NaN bands are pinned in test_nc_gpu.py); here every oracle value has to be a number.
FORMS = ["shared", "unfused", "unshared"]
FUSED_CASES = [(H, bf16, 32, act, "K5", form)                      # every H x tables x form on the plan with hub slots both ways
               for (H, bf16, act) in [(128, False, "sigmoid"), (128, True, "new_sigmoid"), (20, False, "sigmoid"), (20, True, "sigmoid"),
                                      (6, False, "sigmoid"), (6, True, "new_sigmoid")] for form in FORMS]
FUSED_CASES += [(128, True, 512, "new_sigmoid", "K5", "shared"), (20, False, 512, "sigmoid", "K5", "unfused"),              # no slots either way
                (6, False, 512, "sigmoid", "K5", "unshared"),
                (20, True, 32, "new_sigmoid", "K8", "shared"), (20, True, 32, "new_sigmoid", "K8", "unshared")]             # one slice of 8 masks


@pytest.mark.parametrize("H,bf16,chunk,activation,names_key,form", FUSED_CASES,
                         ids=["H%d-%s-c%d-%s-%s-%s" % (c[0], tname(c[1]), c[2], c[3], c[4], c[5]) for c in FUSED_CASES])
def test_fused_halo_against_the_oracle(H, bf16, chunk, activation, names_key, form, monkeypatch):
    from mma_amd import functional as Fn
    pb = fused_problem(H, bf16, activation, names_key)
    graph = plan(chunk)
    assert graph.n_src == S and graph.N == N and (graph.t_n_slots > 0) == (chunk == 32)
    want, truth = fused_oracles(H, bf16, activation, names_key)
    what = "%s/c%d/%s" % (pb.tag, chunk, form)
    assert Fn.SHARED_GRAD_BWD and Fn.FUSE_NODE_BWD
    if form == "shared":
        compare_fused(run_fused(pb, graph), want, truth, pb.names, what)
    elif form == "unfused":
        monkeypatch.setattr(Fn, "FUSE_NODE_BWD", False)
        compare_fused(run_fused(pb, graph), want, truth, pb.names, what)
    else:
        compare_fused(run_fused(pb, graph, reduce_k=False), want, truth, pb.names, what)
        monkeypatch.setattr(Fn, "SHARED_GRAD_BWD", False)
        compare_fused(run_fused(pb, graph), want, truth, pb.names, what + "/reduce_k")


# ---- 2. the std aggregator against the oracle --------------------------------------------------------------------------------------------
STD_CASES = [(H, bf16, chunk, act) for (H, act) in [(128, "sigmoid"), (20, "new_sigmoid"), (6, "sigmoid")] for bf16 in (False, True)
             for chunk in (32, 512)] + [(128, True, 32, "new_sigmoid"), (20, False, 32, "sigmoid"), (6, True, 32, "new_sigmoid")]


@pytest.mark.parametrize("H,bf16,chunk,activation", STD_CASES, ids=["H%d-%s-c%d-%s" % (c[0], tname(c[1]), c[2], c[3]) for c in STD_CASES])
def test_std_halo_against_the_oracle(H, bf16, chunk, activation):
    pb = std_problem(H, bf16, activation)
    graph = plan(chunk)
    want, truth = std_oracles(H, bf16, activation)
    got = run_std(pb, graph)
    assert DEG[1] == 0 and bool((got[0][1].cpu() == float(SQRT_EPS)).all())             # no neighbour: exactly sqrt(1e-5) in fp32
    for g, w, t, name in zip(got, want, truth, ("m", "gx", "gmask_std")):
        compare_one(g, w, t, "%s/c%d/%s" % (pb.tag, chunk, name))


# ---- 3. dropout: the hash takes global edge positions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", list(BASES))
@pytest.mark.parametrize("p_asked,bf16", [(0.5, False), (0.3, True)], ids=["p0.5-fp32", "p0.3-bf16"])
@pytest.mark.parametrize("H", [128, 6])
@pytest.mark.parametrize("kind", ["fused", "std"])
def test_hash_dropout_uses_global_edge_positions(kind, H, p_asked, bf16, base):
    from mma_amd import functional as Fn
    edge_base = BASES[base]
    fused = kind == "fused"
    pb = fused_problem(H, bf16, "sigmoid", "K5") if fused else std_problem(H, bf16, "sigmoid")
    K = pb.K if fused else 1
    keep, p = keep_bits(K, H, p_asked, edge_base)
    keep0, _ = keep_bits(K, H, p_asked, 0)
    # the oracle's mask itself: keyed by the base, and at the rate asked for (K E H >= 8286 bits: 0.02 is four standard deviations)
    assert not np.array_equal(keep, keep0) and abs(float(keep.mean()) - (1.0 - p)) < 0.02
    graph, graph0 = plan(32, edge_base), plan(32, 0)
    assert graph.edge_base == edge_base and graph.edge_base + E < 2 ** 32
    hashed = Fn.DropoutSpec(p_asked, seed=SEED)
    assert hashed.mode == Fn.DROP_HASH and hashed.thr == threshold16(p_asked) and hashed.p_applied == p
    explicit = Fn.DropoutSpec(p, keep=torch.from_numpy(keep).to(DEV))              # indexed by LOCAL edge position
    assert explicit.mode == Fn.DROP_EXPLICIT
    what = "%s/c32/p%g/%s" % (pb.tag, p_asked, base)
    if fused:
        got = run_fused(pb, graph, hashed)
        want, truth = fused_oracles(H, bf16, "sigmoid", "K5", p_asked, edge_base)
        compare_fused(got, want, truth, pb.names, what)
        direct, outputs = fused_direct, ("msum", "gP", "gQ", "gx")
    else:
        got = run_std(pb, graph, hashed)
        want, truth = std_oracles(H, bf16, "sigmoid", p_asked, edge_base)
        for g, w, t, name in zip(got, want, truth, ("m", "gx", "gmask_std")):
            compare_one(g, w, t, what + "/" + name)
        direct, outputs = std_direct, ("m", "gP", "gQ", "gx")
    # what the kernels themselves leave (forward, gP, gQ, gx), bit for bit: the same bits by local position, and another base
    a, b, c = direct(pb, graph, drop=hashed), direct(pb, graph, drop=explicit), direct(pb, graph0, drop=hashed)
    for name in outputs:
        assert torch.equal(a[name], b[name]), "%s: hash mode at edge_base %d and explicit mode with the same bits differ" % (name, edge_base)
        assert not torch.equal(a[name], c[name]), "%s: edge_base does not reach the hash" % name


# ---- the launch helpers, driven directly on caller-owned buffers ---------------------------------------------------------------------------
def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def fused_direct(pb, graph, form="shared", drop=None, parts=False, row_max=False):
    """nc_fwd_launch + nc_bwd_plan on NaN-filled gP (N,KH), gQ (S,KH), gx (S,H) -> dict of everything the kernels wrote."""
    from mma_amd import functional as Fn
    assert Fn.FUSE_NODE_BWD == (form == "shared")
    H, KH = pb.H, pb.K * pb.H
    drop = drop or Fn.DropoutSpec(0.0)
    x = pb.x.to(DEV)
    P = x[:N] @ torch.cat([w[:H] for w in pb.Ws], 1).to(DEV)
    Q = x @ torch.cat([w[H:] for w in pb.Ws], 1).to(DEV)
    if pb.bf16:
        P, Q = Fn.rows_to_bf16(P), Fn.rows_to_bf16(Q)
    g = pb.cot.to(DEV)
    msum, T, sel, crow = Fn.nc_fwd_launch(x, P, Q, graph, pb.kinds, pb.acts, drop, True, True, shared=form != "unshared")
    assert (sel is None) == (form != "unshared") and (crow is None) == (form == "unshared") and msum.shape == (N, H)
    gP, gQ, gx = nan(N, KH), nan(S, KH), nan(S, H)
    rm = torch.zeros((S,), device=DEV) if row_max else None
    gP_out, run = Fn.nc_bwd_plan(x, P, Q, g, T, sel, crow, graph, pb.kinds, pb.acts, drop, True, gP, gQ, gx, rm)
    assert gP_out.data_ptr() == gP.data_ptr()
    if parts:
        halo_part, own_part = graph.t_parts
        run(halo_part)
        run(own_part)
    else:
        run()
    torch.cuda.synchronize()
    return {"msum": msum, "gP": gP, "gQ": gQ, "gx": gx, "row_max": rm, "state": (T, sel, crow)}


def std_direct(pb, graph, drop=None):
    """nc_std_fwd_launch + nc_std_bwd_launch on NaN-filled gP (N,H), gQ (S,H), gx (S,H)."""
    from mma_amd import functional as Fn
    H = pb.H
    drop = drop or Fn.DropoutSpec(0.0)
    x, W = pb.x.to(DEV), pb.W.to(DEV)
    P, Q = x[:N] @ W[:H], x @ W[H:]
    if pb.bf16:
        P, Q = Fn.rows_to_bf16(P), Fn.rows_to_bf16(Q)
    m, saved = Fn.nc_std_fwd_launch(x, P, Q, graph, pb.act, drop, True)
    assert m.shape == (N, H) and saved.shape == (N, 3 * H)
    gP, gQ, gx = nan(N, H), nan(S, H), nan(S, H)
    Fn.nc_std_bwd_launch(x, P, Q, pb.cot.to(DEV), saved, graph, pb.act, drop, gP, gQ, gx)
    torch.cuda.synchronize()
    return {"m": m, "gP": gP, "gQ": gQ, "gx": gx}


def whole_gx(r, Wtop, Wbot):
    """dL/dx on all S rows from what the kernels left: their gx (the direct term + the x_j path) + gP Wtop^T (targets) + gQ Wbot^T, the
    two products in float64 on the CPU."""
    gx = r["gx"].cpu().double() + r["gQ"].cpu().double() @ Wbot.double().t()
    gx[:N] += r["gP"].cpu().double() @ Wtop.double().t()
    return gx.float()


# ---- 4. every row of the caller's buffers is written ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=tname)
@pytest.mark.parametrize("H", [128, 6])
@pytest.mark.parametrize("path", FORMS + ["std"])
def test_every_output_row_is_written(path, H, bf16, monkeypatch):
    """gP (N,.), gQ (S,.), gx (S,H) belong to the caller and come from torch.empty in production: a store the kernels skip leaves
    garbage.  Here they start as NaN."""
    from mma_amd import functional as Fn
    graph = plan(32)
    no_out = torch.from_numpy(NO_OUT).to(DEV)
    assert len(NO_OUT) == 22 and OUT_DEG[291] == 0
    if path == "std":
        pb = std_problem(H, bf16, "sigmoid")
        r = std_direct(pb, graph)
        for name in ("m", "gP", "gQ", "gx"):
            assert not bool(torch.isnan(r[name]).any()), "an element of %s was not written" % name
        assert not bool(r["gQ"][no_out].any()) and not bool(r["gx"][no_out].any())      # std has no self term: no out-edge, no gradient at all
        assert not bool(r["gP"][1].any()) and not bool(r["gP"][2].any())                # the zero cotangent of the degenerate targets
        want, truth = std_oracles(H, bf16, "sigmoid")
        compare_one(r["m"], want[0], truth[0], pb.tag + "/direct/m")
        compare_one(whole_gx(r, pb.W[:H], pb.W[H:]), want[1], truth[1], pb.tag + "/direct/gx")
        return
    pb = fused_problem(H, bf16, "sigmoid", "K5")
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", path == "shared")
    r = fused_direct(pb, graph, path)
    for name in ("msum", "gP", "gQ", "gx"):
        assert not bool(torch.isnan(r[name]).any()), "%s: an element of %s was not written" % (path, name)
    assert not bool(r["gQ"][no_out].any())                                          # no out-edge: a row of exact zeros
    assert not bool(r["gx"][291].any())                                             # ... and, with no target role either, in gx too
    # an own source with no out-edge: the direct (combine) term alone - what K2a leaves in gxs from the same saved state ...
    T, sel, crow = r["state"]
    _, _, gxs = Fn.nc_bwd_node_launch(pb.cot.to(DEV), True, sel, crow, T, graph, pb.kinds, H, crow is not None)
    torch.cuda.synchronize()
    assert not bool(gxs[N:].any()) and bool(torch.isfinite(gxs).all())
    rows = torch.from_numpy(NO_OUT_OWN).to(DEV)
    check_close(r["gx"][rows], gxs[rows].cpu().numpy(), None, None, what="%s/%s/direct term of the sources without out-edge" % (pb.tag, path))
    # ... and, once gP Wtop^T and gQ Wbot^T are added, the oracle's rows (theirs among all S)
    want, truth = fused_oracles(H, bf16, "sigmoid", "K5")
    Wtop, Wbot = torch.cat([w[:H] for w in pb.Ws], 1), torch.cat([w[H:] for w in pb.Ws], 1)
    compare_one(r["msum"], want["msum"], truth["msum"], "%s/%s/direct/msum" % (pb.tag, path))
    compare_one(whole_gx(r, Wtop, Wbot), want["gx"], truth["gx"], "%s/%s/direct/gx" % (pb.tag, path))


# ---- 5. the backward in two launches over t_parts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shared", "unfused"])
@pytest.mark.parametrize("bf16", [False, True], ids=tname)
@pytest.mark.parametrize("H", [128, 20])
def test_backward_in_two_parts_equals_one_launch(H, bf16, form, monkeypatch):
    """run(halo_part); run(own_part) - what the sharded layer does around its reverse exchange - against run() on fresh buffers."""
    from mma_amd import functional as Fn
    pb = fused_problem(H, bf16, "sigmoid", "K5")
    graph = plan(32, BASES["base12345"])
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", form == "shared")
    drop = Fn.DropoutSpec(0.5, seed=SEED)
    one = fused_direct(pb, graph, form, drop, parts=False, row_max=True)
    two = fused_direct(pb, graph, form, drop, parts=True, row_max=True)
    for name in ("gP", "gQ", "gx", "row_max"):
        assert not bool(torch.isnan(two[name]).any()), name
        assert torch.equal(one[name], two[name]), "%s differs between one launch and the two parts" % name
    assert float(one["row_max"][N:].max()) > 0


# ---- 6. the row maxima, halo rows included ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shared", "unfused"])
@pytest.mark.parametrize("H,bf16,p_asked", [(128, False, 0.5), (20, True, 0.0), (6, True, 0.3)], ids=["H128-fp32-p0.5", "H20-bf16-p0", "H6-bf16-p0.3"])
def test_row_maxima_on_halo_rows(H, bf16, p_asked, form, monkeypatch):
    """row_max[j] = max |[gP | gQ][j, :]| for a target row, max |gQ[j, :]| for a halo row: taken over exactly the stored values, so
    equality is the contract (test_nc_layer_paths_gpu.py: test_row_maxima_equal_the_rows_they_stand_for)."""
    from mma_amd import functional as Fn
    pb = fused_problem(H, bf16, "sigmoid", "K5")
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", form == "shared")
    r = fused_direct(pb, plan(32), form, Fn.DropoutSpec(p_asked, seed=SEED), row_max=True)
    assert bool(torch.isfinite(r["gP"]).all()) and bool(torch.isfinite(r["gQ"]).all()) and bool(torch.isfinite(r["gx"]).all())
    want = r["gQ"].abs().amax(1)
    want[:N] = torch.maximum(want[:N], r["gP"].abs().amax(1))
    rm = r["row_max"]
    bad = torch.nonzero(rm != want).flatten()
    assert bad.numel() == 0, "row_max != max|row| on %d rows, first %d: %r vs %r" % (bad.numel(), int(bad[0]), float(rm[bad[0]]), float(want[bad[0]]))
    assert float(rm[291]) == 0.0                                                    # a halo row with no out-edge: exactly 0 ("skip the row")
    assert int((rm == 0).sum()) < S // 2 and float(rm[N:].max()) > 0 and float(rm[:N].max()) > 0


# ---- 7. no atomics on these paths: a second run gives the same bits ----------------------------------------------------------------------------
def test_runs_repeat_bit_for_bit():
    from mma_amd import functional as Fn
    graph = plan(32, BASES["base12345"])
    drop = Fn.DropoutSpec(0.3, seed=SEED)
    fused, std = fused_problem(20, True, "sigmoid", "K5"), std_problem(20, False, "sigmoid")
    a, b = fused_direct(fused, graph, drop=drop), fused_direct(fused, graph, drop=drop)
    for name in ("msum", "gP", "gQ", "gx"):
        assert torch.equal(a[name], b[name]), "fused: " + name
    a, b = std_direct(std, graph, drop), std_direct(std, graph, drop)
    for name in ("m", "gP", "gQ", "gx"):
        assert torch.equal(a[name], b[name]), "std: " + name
