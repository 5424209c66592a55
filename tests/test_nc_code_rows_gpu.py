"""GPU tests of the packed code rows of the fused NC kernels (include/mma_amd.h ABI 41, csrc/nc_fused.hip): K1 leaves, per target,
[1/d, 0, 0, 0 | per max/min/softmax-type mask a slot of 2 bits per element], and K2b (per edge), its epilogue, K2a and the hub sums
read it.  Element c of a slot lives in byte c/4 at bits 2(c%4) whatever vector width wrote or reads it.

Everything is compared with the float64 oracle at the project's bar (golden_util.check_close with truth, as the other NC files do): the
fused aggregators restated in torch (test_nc_bf16_gpu.fused_oracle), float64 the truth, float32 the reference value.  One graph
(code_graph) carries what the format can get wrong:
  * a hub target and two hub sources (an own and a halo one) cut into chunks of 32: the hub sums write and read code rows too;
  * targets of degree 1 whose one source is a copy of their own row, with zeros in every third column: s == x_i == 0 there in every
    arithmetic - exact ties (the code of "half / half") - and s != x_i elsewhere;
  * a target whose sources are huge in the first columns, so that softmax's exp(s) overflows: the code of the NaN gradient.  The mask
    weights are zero on those columns, so the logits stay ordinary and s is far above the overflow point (asserted);
  * the halo form: 160 targets over 200 source rows.  The same graph as an ordinary 200-node one (rows >= 160 take no in-edge) runs the
    one-launch form, which the halo form does not have.
Widths: H = 1, 3, 4, 5 (lanes that share a byte, a last byte partly used), 8, 20, 36 (slot rounding), 128, 132 (one and two column
blocks; VEC = 4 and VEC = 1).  Mask sets with zero, one, two and eight code slots."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from golden_util import check_close
from nc_layer_util import BF16, DEV, csr_of, embed, rounded
from test_nc_bf16_gpu import fused_oracle
from oracle import nc_oracle as O

pytestmark = pytest.mark.gpu
F32 = torch.float32
WIDTHS = [1, 3, 4, 5, 8, 20, 36, 128, 132]
MASK_SETS = {"none": ["sum", "mean"], "one": ["max"], "two": ["sum", "mean", "max", "min"],
             "eight": ["max", "max2", "max3", "max4", "min", "min2", "min3", "min4"], "nan": ["softmax", "min"]}
SEL_KINDS = ("max", "min", "softmax", "softmin")
N, S = 160, 200
HUB_T, HUB_S, HUB_S_HALO, NAN_T = 0, 1, 191, 10
TWINS = {t: (180 + t if t < 6 else 140 + t) for t in range(2, 10)}          # degree-1 target -> its one source (halo: 182..185, own: 146..149)
NAN_SRC = list(range(192, 200))
EXP_OVERFLOW = 88.72                                                            # expf(s) is inf above it
tname = lambda bf16: "bf16" if bf16 else "fp32"


def code_graph():
    rng = np.random.default_rng(41)
    edges = {(HUB_T, s) for s in range(90, 190)}                                # 100 sources, own and halo
    edges |= {(t, HUB_S) for t in range(20, 120)} | {(t, HUB_S_HALO) for t in range(30, 130)}
    edges |= {(t, s) for t, s in TWINS.items()} | {(NAN_T, s) for s in NAN_SRC}
    for t in range(11, N):
        for s in rng.choice(np.arange(11, 190), size=rng.integers(0, 6), replace=False):
            edges.add((t, int(s)))
    return [sorted(s for (t, s) in edges if t == i) for i in range(N)]


ADD = code_graph()
FULL = embed(ADD, S)
DEG, COL = csr_of(ADD)
ROWPTR = np.concatenate([[0], np.cumsum(DEG)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def plan(halo):
    """chunk 32: the hubs take 4 slots each.  halo: N targets over S sources; else the same graph on S nodes."""
    import mma_amd
    if halo:
        return mma_amd.NCGraph(ROWPTR, COL, DEV, n_src=S, chunk=32, group_below=8, t_group_below=8)
    rowptr = np.concatenate([ROWPTR, np.full(S - N, ROWPTR[-1])])
    return mma_amd.NCGraph(rowptr, COL, DEV, chunk=32, group_below=8, t_group_below=8)


class Problem:
    def __init__(self, H, masks, bf16):
        from mma_amd import functional as Fn
        self.H, self.bf16, self.names = H, bf16, MASK_SETS[masks]
        self.K = len(self.names)
        rng = np.random.default_rng(500 + H)
        u = lambda: (rng.random((2 * H, H)) * 2 - 1) / np.sqrt(H)
        if bf16:      # the grids of test_nc_bf16_gpu.py: P and Q are exact, so the three sides round the same tables
            x = rng.integers(-32, 33, (S, H)) / 32.0
            Ws = [np.round(u() * 512.0) / 512.0 for _ in self.names]
        else:         # as test_nc_gpu.py draws them, at half the size
            x = 0.5 * np.maximum(rng.standard_normal((S, H)), 0)
            Ws = [u() for _ in self.names]
        for t, s in TWINS.items():
            x[t, 0::3] = 0
            x[s] = x[t]
        self.big = min(2, H)
        x[NAN_SRC, :self.big] = 64.0                # 8 sources: s = 64 * sum of 8 sigmoids
        for W in Ws:                                # the huge columns stay out of the logits
            W[:self.big] = 0
            W[H:H + self.big] = 0
        self.x = torch.from_numpy(x.astype(np.float32))
        self.Ws = [torch.from_numpy(W.astype(np.float32)) for W in Ws]
        cot = rng.standard_normal((S, H)).astype(np.float32)
        cot[N:] = 0                                 # rows >= N are sources only
        self.cot = torch.from_numpy(cot)
        self.kinds = [Fn.KIND[O.AGGREGATORS[n][0]] for n in self.names]
        self.acts = [Fn.ACT_SIGMOID] * self.K
        self.table_dtype = BF16 if bf16 else F32
        self.tag = "crow/H%d/%s/%s" % (H, masks, tname(bf16))


@functools.lru_cache(maxsize=None)
def problem(H, masks, bf16):
    return Problem(H, masks, bf16)


@contextlib.contextmanager
def one_thread():
    """The oracle's tensors have a few hundred rows: torch's CPU thread pool only adds its hand-over to every index_add (measured: 20x
    the time with 8 threads)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def oracles(H, masks, bf16):
    """(float32 reference, float64 truth) on the S-node graph, once: m (K,S,H), msum, gx and the mask-weight gradients of <msum, cot>."""
    pb = problem(H, masks, bf16)
    out = []
    with one_thread():
        for dt in (F32, torch.float64):
            xo = pb.x.clone().to(dt).requires_grad_(True)             # clone: .to() of the same dtype is the problem's own tensor
            Wo = [w.clone().to(dt).requires_grad_(True) for w in pb.Ws]
            m = fused_oracle(xo, Wo, pb.names, FULL, "sigmoid", None, 0.0, pb.table_dtype)
            g = torch.autograd.grad((m.sum(0) * pb.cot.to(dt)).sum(), [xo] + Wo)
            n = lambda t: t.detach().numpy()
            out.append({"m": n(m), "msum": n(m.sum(0)), "gx": n(g[0]), "gmask": [n(a) for a in g[1:]]})
    return tuple(out)


def neighbour_sums(pb, k):
    """s (S,H) of mask k in float64: the oracle's own statement (fused_oracle) up to the combine."""
    x, W, H = pb.x.double(), pb.Ws[k].double(), pb.H
    dst, col = torch.from_numpy(np.repeat(np.arange(N), DEG)), torch.from_numpy(COL)
    P, Q = rounded(x @ W[:H], pb.table_dtype), rounded(x @ W[H:], pb.table_dtype)
    with one_thread():
        return torch.zeros(S, H, dtype=torch.float64).index_add(0, dst, torch.sigmoid(P[dst] + Q[col]) * x[col]).numpy()


def oracle_codes(pb, k):
    """The 2-bit codes of mask k (a max/min/softmax kind) the oracle derives, 2 * dm/ds: (codes (N,H), sure (N,H)); `sure` is False
    where s and x_i are closer than fp32 can tell apart without being equal (nowhere, or almost: asserted by the caller)."""
    s, x = neighbour_sums(pb, k)[:N], pb.x.double().numpy()[:N]
    kind = pb.names[k].rstrip("234")
    if kind in ("softmax", "softmin"):
        a = s if kind == "softmax" else -s
        return np.where(a > EXP_OVERFLOW, 3, 2), np.abs(a - EXP_OVERFLOW) > 1.0
    sel = s > x if kind == "max" else s < x
    return np.where(sel, 2, np.where(s == x, 1, 0)), (s == x) | (np.abs(s - x) > 1e-5 * np.maximum(1.0, np.abs(s)))


def front_bytes(H, kinds):
    """The live front of a code row: the 16-byte header and, per code slot (a max/min/softmax kind), 2 bits per element rounded up to 4 bytes."""
    return 16 + sum(k >= 2 for k in kinds) * 4 * -(-H // 16)


def decode(crow, slot, H):
    """The codes (N,H) of one slot of the code rows (the float32 tensor (N,ldc) K1 wrote) in numpy."""
    b = crow.view(torch.uint8).cpu().numpy()
    sb = 4 * -(-H // 16)
    c = np.arange(H)
    return (b[:, 16 + slot * sb + c // 4] >> (2 * (c % 4))) & 3


def compare_one(got, want, truth, what):
    g = got.detach().cpu().numpy().astype(np.float64)
    print("%s: max |got - fp64| %.3g, max |fp32 ref - fp64| %.3g" % (what, np.nanmax(np.abs(g - truth)), np.nanmax(np.abs(want.astype(np.float64) - truth))))
    check_close(got, want, None, None, what=what, signed_sum=True, truth=truth)


def run_layer_path(pb, graph):
    """nc_fused_aggregate (reduce_k: the shared-gradient backward on the code rows) with P / Q by torch -> msum, gx, gmask."""
    from mma_amd import functional as Fn
    H, n = pb.H, graph.N
    xg = pb.x.to(DEV).requires_grad_(True)
    Wg = [w.to(DEV).requires_grad_(True) for w in pb.Ws]
    P = xg[:n] @ torch.cat([w[:H] for w in Wg], 1)
    Q = xg @ torch.cat([w[H:] for w in Wg], 1)
    out = Fn.nc_fused_aggregate(xg, P, Q, graph, pb.kinds, pb.acts, None, reduce_k=True, logit_dtype=BF16 if pb.bf16 else None)
    assert out.shape == (n, H)
    g = torch.autograd.grad((out * pb.cot[:n].to(DEV)).sum(), [xg] + Wg)
    torch.cuda.synchronize()
    return {"msum": out.detach(), "gx": g[0], "gmask": list(g[1:])}


def compare(got, H, masks, bf16, what):
    pb = problem(H, masks, bf16)
    want, truth = oracles(H, masks, bf16)
    n = got["msum"].shape[0]
    compare_one(got["msum"], want["msum"][:n], truth["msum"][:n], what + "/msum")
    compare_one(got["gx"], want["gx"], truth["gx"], what + "/gx")
    for k, name in enumerate(pb.names):
        compare_one(got["gmask"][k], want["gmask"][k], truth["gmask"][k], "%s/gmask[%s]" % (what, name))


# ---- the graph and the problems reach what they are for (no kernel runs) -----------------------------------------------------------------
def test_the_graph_reaches_the_paths():
    g = plan(True)
    assert (g.N, g.n_src, g.E) == (N, S, int(ROWPTR[-1])) and g.E < 1000
    assert DEG[HUB_T] == 100 and all(DEG[t] == 1 for t in TWINS) and DEG[NAN_T] == len(NAN_SRC)
    assert g.hubs[:, 0].tolist() == [HUB_T] and g.n_slots == 4                                   # K1's hub sums
    assert g.t_hubs[:, 0].tolist() == [HUB_S, HUB_S_HALO] and g.t_n_slots == 8                     # K2b's: a target (epilogue) and a halo source
    assert 0 < g.n_wave_items < g.items.shape[0] and 0 < g.t_n_wave_items < g.t_items.shape[0]     # wavefront items and grouped items
    flat = plan(False)
    assert (flat.N, flat.n_src) == (S, S) and flat.n_slots == 4 and flat.t_n_slots == 8


@pytest.mark.parametrize("bf16", [False, True], ids=tname)
@pytest.mark.parametrize("H", WIDTHS)
def test_the_problems_hold_every_code(H, bf16):
    pb = problem(H, "eight", bf16)
    codes, sure = oracle_codes(pb, 0)                                   # max
    assert sure.all() and set(np.unique(codes)) == {0, 1, 2}
    assert (codes[list(TWINS)][:, 0::3] == 1).all()                     # the exact ties
    pb = problem(H, "nan", bf16)
    codes, sure = oracle_codes(pb, 0)                                   # softmax
    assert sure.all()
    assert (codes[NAN_T, :pb.big] == 3).all() and (codes == 3).sum() == pb.big              # there and nowhere else
    want, truth = oracles(H, "nan", bf16)
    assert np.array_equal(np.isnan(want["m"][0]), np.pad(codes == 3, ((0, S - N), (0, 0)))) and np.isfinite(truth["m"]).all()


# ---- 1. every width x mask set x form against the oracle ------------------------------------------------------------------------------------
CASES = [(H, masks, False) for H in WIDTHS for masks in MASK_SETS] + [(H, masks, True) for H in WIDTHS for masks in ("two", "eight", "nan")]


@pytest.mark.parametrize("H,masks,bf16", CASES, ids=["H%d-%s-%s" % (c[0], c[1], tname(c[2])) for c in CASES])
def test_against_the_oracle(H, masks, bf16, monkeypatch):
    """halo form: K2a in K2b's epilogue, K2a as a launch of its own (the separate launches).  The same graph on S nodes: the separate
    launches, and the one-launch small form (taken where the rows are vectors: H % 4 == 0) with K2a either way."""
    from mma_amd import functional as Fn, graph as G
    pb = problem(H, masks, bf16)
    assert Fn.SHARED_GRAD_BWD and Fn.FUSE_NODE_BWD
    halo, flat = plan(True), plan(False)
    compare(run_layer_path(pb, halo), H, masks, bf16, pb.tag + "/halo/epilogue")
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", False)
    compare(run_layer_path(pb, halo), H, masks, bf16, pb.tag + "/halo/unfused")
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", True)
    monkeypatch.setattr(G, "ONE_LAUNCH", False)
    assert flat.sync(0) is None
    compare(run_layer_path(pb, flat), H, masks, bf16, pb.tag + "/flat/two-launch/epilogue")
    if H % 4 == 0:
        monkeypatch.setattr(G, "ONE_LAUNCH", True)
        assert flat.sync(0) is not None and flat.sync(1) is not None
        compare(run_layer_path(pb, flat), H, masks, bf16, pb.tag + "/flat/one-launch/epilogue")
        monkeypatch.setattr(Fn, "FUSE_NODE_BWD", False)
        compare(run_layer_path(pb, flat), H, masks, bf16, pb.tag + "/flat/one-launch/unfused")
        assert int(flat._sync.abs().sum()) == 0


# ---- the kernels driven directly on caller-owned buffers -----------------------------------------------------------------------------------
def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def odd_pitch(t):
    """The same (rows, cols) values as a column block of a buffer one element wider: a pitch that is no multiple of 4 sends an entry
    point to its scalar (VEC = 1) kernels."""
    buf = torch.zeros((t.shape[0], t.shape[1] + 1), device=t.device, dtype=t.dtype)
    buf[:, :-1] = t
    v = buf[:, :-1]
    assert v.stride(0) % 4 != 0 and v.stride(1) == 1
    return v


def direct(x, P, Q, g, kinds, acts, graph, fwd_scalar=False, bwd_scalar=False, fill_from=None):
    """nc_fwd_launch + nc_bwd_plan -> everything the kernels wrote.  fwd_scalar: K1 reads P at an odd pitch; bwd_scalar: K2b writes gQ at
    one; fill_from: the bytes of every code row from that offset on are set to 0xFF between the two."""
    from mma_amd import functional as Fn
    n, KH, H = graph.N, P.shape[1], x.shape[1]
    drop = Fn.DropoutSpec(0.0)
    msum, T, sel, crow = Fn.nc_fwd_launch(x, odd_pitch(P) if fwd_scalar else P, Q, graph, kinds, acts, drop, True, True)
    assert sel is None and tuple(crow.shape) == (n, Fn.crow_floats(H, kinds))
    # what K1 wrote of the rows: 1/d and the codes (floats 1..3, the bytes that round a slot up to 4 and everything behind the slots
    # are never written: whatever torch.empty left)
    n_sel = sum(k >= 2 for k in kinds)
    state = {"inv_deg": crow[:, 0].clone(), "slots": crow.view(torch.uint8)[:, 16:front_bytes(H, kinds)].clone(),
             "codes": torch.from_numpy(np.stack([decode(crow, slot, H) for slot in range(n_sel)]))}
    if fill_from is not None:
        crow.view(torch.uint8)[:, fill_from:] = 0xFF
    gP, gx = nan(n, KH), nan(graph.n_src, H)
    gQ = odd_pitch(nan(graph.n_src, KH)) if bwd_scalar else nan(graph.n_src, KH)
    _, run = Fn.nc_bwd_plan(x, P, Q, g, T, sel, crow, graph, kinds, acts, drop, True, gP, gQ, gx)
    run()
    torch.cuda.synchronize()
    return dict(state, msum=msum, T=T, gP=gP, gQ=gQ.contiguous(), gx=gx)


# ---- 2. a scalar-path writer feeds a vector-path reader, and the reverse ---------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [True, False], ids=["epilogue", "unfused"])
@pytest.mark.parametrize("bf16", [False, True], ids=tname)
@pytest.mark.parametrize("H", [4, 8, 132])
def test_writer_and_reader_on_different_paths(H, bf16, fuse, monkeypatch):
    """Forward and backward choose their vector width from different pointers and pitches.  The two widths walk an item with a
    different number of lanes per row, so they add the edges up in a different order; for the results to be comparable bit for bit the
    inputs are such that every sum is exact in fp32 whatever its order: raw logits (a = z, a' = 1) with P, Q and the cotangent in
    multiples of 1/8 within [-1, 1], x in multiples of 1/32 - a term has at most 11 bits, a sum over at most 100 edges 18.
    [sum, max, min, softmax]: e / e = 1 exactly, and the twins tie where both are zero.  H = 132 beside 4 and 8: there the scalar
    kernels walk a row in three column blocks of 64 lanes, the vector kernels in one."""
    from mma_amd import functional as Fn
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", fuse)
    rng = np.random.default_rng(900 + H)
    names = ["sum", "max", "min", "softmax"]
    kinds, acts = [Fn.KIND[O.AGGREGATORS[n][0]] for n in names], [Fn.ACT_RAW] * 4
    x = rng.integers(-32, 33, (S, H)) / 32.0
    for t, s in TWINS.items():
        x[t, 0::3] = 0
        x[s] = x[t]
    eighths = lambda *shape: torch.from_numpy((rng.integers(-8, 9, shape) / 8.0).astype(np.float32)).to(DEV)
    x = torch.from_numpy(x.astype(np.float32)).to(DEV)
    P, Q, g = eighths(N, 4 * H), eighths(S, 4 * H), eighths(N, H)
    if bf16:
        P, Q = P.to(BF16), Q.to(BF16)               # multiples of 1/8: exact
    graph = plan(True)
    ref = direct(x, P, Q, g, kinds, acts, graph)
    codes = ref["codes"].numpy()
    assert all(set(np.unique(c)) <= {0, 1, 2} for c in codes) and (codes[0] == 1).any() and (codes[1] == 1).any() and (codes[2] == 2).all()
    assert bool(torch.isfinite(ref["gx"]).all())
    for name, kw in (("scalar forward, vector backward", dict(fwd_scalar=True)), ("vector forward, scalar backward", dict(bwd_scalar=True)),
                     ("both scalar", dict(fwd_scalar=True, bwd_scalar=True))):
        got = direct(x, P, Q, g, kinds, acts, graph, **kw)
        for key in ref:
            if key != "slots":          # at these widths a slot has bytes no element lives in
                assert torch.equal(got[key], ref[key]), "%s: %s differs from the all-aligned run" % (name, key)


# ---- 3. the packed front of the row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=tname)
def test_packed_front_at_the_flagship_width(bf16, monkeypatch):
    """H = 128, [sum, mean, max, min]: bytes 0..3 are 1/d, bytes 16..47 the codes of max, 48..79 those of min - the selection
    the oracle derives - and nothing reads a byte from 80 on: filled with 0xFF before the backward, the gradients are the same bits,
    with K2a in the epilogue and as a launch of its own (the hub sums of both directions included)."""
    from mma_amd import functional as Fn
    H, KH = 128, 4 * 128
    pb = problem(H, "two", bf16)
    graph = plan(True)
    x = pb.x.to(DEV)
    P = x[:N] @ torch.cat([w[:H] for w in pb.Ws], 1).to(DEV)
    Q = x @ torch.cat([w[H:] for w in pb.Ws], 1).to(DEV)
    if bf16:
        P, Q = Fn.rows_to_bf16(P), Fn.rows_to_bf16(Q)
    g = pb.cot[:N].to(DEV)
    assert Fn.crow_floats(H, pb.kinds) * 4 == 272
    for fuse in (True, False):
        monkeypatch.setattr(Fn, "FUSE_NODE_BWD", fuse)
        ref = direct(x, P, Q, g, pb.kinds, pb.acts, graph)
        got = direct(x, P, Q, g, pb.kinds, pb.acts, graph, fill_from=80)
        for key in ref:
            assert torch.equal(got[key], ref[key]), "%s differs once the bytes from 80 on are 0xFF (K2a %s)" % (key, "fused" if fuse else "unfused")
        assert bool(torch.isfinite(ref["gP"]).all() and torch.isfinite(ref["gQ"]).all() and torch.isfinite(ref["gx"]).all())
    assert ref["slots"].shape == (N, 64)                    # bytes 16..79
    assert np.array_equal(ref["inv_deg"].cpu().numpy(), np.float32(1.0) / np.maximum(DEG, 1).astype(np.float32))
    for slot, k in ((0, 2), (1, 3)):
        want, sure = oracle_codes(pb, k)
        assert sure.mean() > 0.999 and {0, 1, 2} == set(np.unique(want))
        c = np.arange(H)
        got = (ref["slots"].cpu().numpy()[:, 32 * slot + c // 4] >> (2 * (c % 4))) & 3
        assert np.array_equal(got[sure], want[sure]), "slot %d (%s): %d codes differ from the oracle's selection" % (slot, pb.names[k], (got != want)[sure].sum())
