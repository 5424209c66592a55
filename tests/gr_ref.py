"""Plain reference and direct-call driver for K3 / K4 (mma_gr_fused_fwd / mma_gr_fused_bwd), shared by tests/test_gr_forms_gpu.py.

Layout: a target-sorted edge list built from a DEGREE LIST (node n gets deg[n] edges), then shuffled as PyG hands it over; the stable
sort of mma_build_csr puts a node's edges back in ascending original id, so `Layout.edge(n, k)` - the k-th smallest edge id of node n -
is the edge at OFFSET k of n's segment, the number the saved args hold.

Reference: the fused message in numpy float32 in the kernels' own association, ((V[j] + U[i]) + Z[r]) * f, with f from
oracle.dropout_rng.keep_mask16 over the whole width D keyed by the original edge id - exact, so min / max and their args are bit for bit
the kernels'; the aggregation by oracle.gr_oracle.aggregate in float32 and in float64 (the truth of golden_util.check_close's noise bar);
the arg by gr_oracle.scatter_sequential (small cases) or by `arg_offsets_vectorised` (the large ones; the two are compared where both
run).

Driver: `run` calls K3 and K4 through functional._gr_call on caller-owned buffers whose every output is pre-filled (NaN, the byte
SENT8, the int SENT32), after asserting with functional.gr_plan that each call takes the kernels the case names."""
import numpy as np
import torch

from mma_amd import functional as Fn
from mma_amd.functional import GR_AGGR, GR_SCALER
from mma_amd._lib import ptr
from oracle import gr_oracle as G
from oracle.dropout_rng import keep_mask16, threshold16

DEV = "cuda:0"
SENT8, SENT32 = 0xEE, -7777
AVG = {"log": 1.25, "lin": 2.0}                   # the degree statistics of the scalers (exact in fp32)


class Layout:
    """deg (N,) -> the shuffled edge list (src, dst by original id) and what the stable sort by target makes of it."""

    def __init__(self, deg, rng):
        deg = np.asarray(deg, np.int64)
        self.deg, self.N, self.E = deg, len(deg), int(deg.sum())
        seg = np.repeat(np.arange(self.N), deg)
        sh = rng.permutation(self.E)
        self.dst = seg[sh]
        self.src = rng.integers(0, self.N, self.E)
        self.perm = np.argsort(self.dst, kind="stable")              # position -> original edge id
        self.pos = np.empty(self.E, np.int64)
        self.pos[self.perm] = np.arange(self.E)                      # original edge id -> position
        self.rowptr = np.concatenate([[0], np.cumsum(deg)])
        self.seg = seg                                               # position -> node

    def edge(self, n, k):
        return int(self.perm[self.rowptr[n] + k])

    def edge_index(self):
        return np.stack([self.src, self.dst])

    def offsets(self):
        """position -> offset inside its segment"""
        return np.arange(self.E) - self.rowptr[self.seg]


def drop_factor(p, seed, E, D):
    """(E, D) float32: 0 or 65536 / (65536 - thr16) as the kernels form it, by original edge id; None for p == 0."""
    if p == 0:
        return None
    thr = threshold16(p)
    keep = keep_mask16(seed, thr, 1, E, D)[0]
    return keep.astype(np.float32) * (np.float32(65536.0) / np.float32(65536 - thr))


def fused_sum(L, U, V, Z, zidx=None):
    """(V[j] + U[i]) + Z[r] in float32, rows by original edge id.  Z: (E, D) by original id, a table with zidx (E,), or None."""
    s = V[L.src] + U[L.dst]
    if Z is not None:
        s = s + (Z[zidx] if zidx is not None else Z)
    return s.astype(np.float32)


def reference(L, s, fac, T, F, aggs, scalers, gouts):
    """s (E, D) float32: the given messages, or the fused sum before dropout; fac (E, D) or None.  -> dict of float32 results and their
    float64 truths: out (N, T, S*K*F), and per gout: gmsg (E, D) = dL/ds by original id, gU (N, D) = its sum over each target."""
    res = {}
    idx = torch.from_numpy(L.dst)
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        st = torch.from_numpy(s).to(dt).requires_grad_(True)
        h = st if fac is None else st * torch.from_numpy(fac).to(dt)
        out = G.aggregate(h.view(L.E, T, F), idx, L.N, aggs, scalers, AVG)
        res["out" + name] = out.detach().numpy()
        res["gmsg" + name], res["gU" + name] = [], []
        for g in gouts:
            if L.E:
                gm, = torch.autograd.grad((out * torch.from_numpy(g).to(dt)).sum(), [st], retain_graph=True)
            else:
                gm = torch.zeros_like(st)
            res["gmsg" + name].append(gm.numpy())
            res["gU" + name].append(torch.zeros((L.N, T * F), dtype=dt).index_add(0, idx, gm).numpy())
    return res


def arg_offsets(L, h, red):
    """(N, D) offsets of the extremal edge of every (node, column) from gr_oracle.scatter_sequential; -1: no edge."""
    _, arg = G.scatter_sequential(h, L.dst, L.N, red)
    off = np.where(arg >= 0, L.pos[np.maximum(arg, 0)] - L.rowptr[:-1, None], -1)
    return off


def arg_offsets_vectorised(L, h, red):
    """The same without a loop over edges: the lowest offset whose value equals the segment's extremum."""
    D = h.shape[1]
    hp = h[L.perm]                                                   # position order
    ext = np.full((L.N, D), np.inf if red == "min" else -np.inf, np.float32)
    (np.minimum if red == "min" else np.maximum).at(ext, L.seg, hp)
    cand = np.where(hp == ext[L.seg], L.offsets()[:, None], 1 << 30)
    off = np.full((L.N, D), 1 << 30, np.int64)
    np.minimum.at(off, L.seg, cand)
    return np.where(off == 1 << 30, -1, off)


def scaler_products(deg, scalers):
    """(N, S) float64: the running product of the degree scalers at every node (degree clamped to 1), as aggregate() compounds them"""
    d = np.maximum(np.asarray(deg, np.float64), 1.0)
    fac = {"identity": np.ones_like(d), "amplification": np.log(d + 1) / AVG["log"], "attenuation": AVG["log"] / np.log(d + 1),
           "linear": d / AVG["lin"], "inverse_linear": AVG["lin"] / d}
    return np.cumprod(np.stack([fac[s] for s in scalers], 1), 1)


def node_bounds(L, T, F, aggs, scalers, gout, p):
    """The bound K4's block kernel documents for the message-gradient rows of a node: every such row is, column by column,
    keep * (c_all + [arg hit] c_min + [arg hit] c_max) with c_k = sum over the scaler blocks q of (running scaler product) * gout (mean:
    / deg), so max |row| <= scale * max_c (|c_all| + |c_min| + |c_max|).  Float64 -> (bound (N,), slack (N,)); the slack is 1e-5 of the
    same expression over the absolute terms: what fp32 sums of at most eight products can be off by, with a wide margin."""
    K, S = len(aggs), len(scalers)
    g = np.asarray(gout, np.float64).reshape(L.N, T, S, K, F)
    pre = scaler_products(L.deg, scalers)[:, None, :, None]                               # (N, 1, S, 1)
    d = np.maximum(L.deg, 1).astype(np.float64)[:, None, None]
    zero = np.zeros((L.N, T, F))
    parts = {"all": [zero, zero], "min": [zero, zero], "max": [zero, zero]}               # [signed sum, sum of absolute terms]
    for k, a in enumerate(aggs):
        term = g[:, :, :, k] * pre
        if a == "mean":
            term = term / d[:, :, None]
        key = a if a in ("min", "max") else "all"
        assert a in ("sum", "mean", "min", "max")
        parts[key] = [parts[key][0] + term.sum(2), parts[key][1] + np.abs(term).sum(2)]
    thr = threshold16(p) if p > 0 else 0
    scale = 65536.0 / (65536.0 - thr)
    bound = scale * sum(np.abs(v[0]) for v in parts.values()).reshape(L.N, -1).max(1)
    mag = scale * sum(v[1] for v in parts.values()).reshape(L.N, -1).max(1)
    return bound, 1e-5 * mag


def onehot_gout(N, T, F, K, S, k, q=0):
    """A cotangent that is 1 on aggregator k's block of scaler q and 0 elsewhere."""
    g = np.zeros((N, T, S, K, F), np.float32)
    g[:, :, q, k] = 1.0
    return g.reshape(N, T, S * K * F)


def _padded(rows, width, pad, fill=float("nan"), dtype=torch.float32, shift=0):
    """A (rows, width) view with row pitch width + pad inside a pre-filled buffer; shift: elements the view starts into the buffer."""
    ld = width + pad
    buf = torch.full((rows * ld + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf.as_strided((rows, width), (ld, 1), shift)


class Result:
    pass


def run(L, T, F, aggs, scalers, gouts, *, inputs=None, U=None, V=None, Z=None, zidx=None, by_pos=False, p=0.0, seed=0x5EED, with_list=True,
        pad_uv=0, pad_z=0, pad_save=0, pad_g=0, pad_gu=0, u_shift=0, row_max=False, expect=None, graph=None):
    """One K3 call and one K4 call per cotangent of `gouts`.  Operands are numpy arrays by original edge id (`Z` (E, D), or a table with
    `zidx`); with by_pos the Z rows / index bytes go to the device in position order and gmsg comes back in position order.  pad_*: extra
    floats of row pitch (lduv = 2 D + pad_uv, ldz, ldsave, ldg = D + pad, ldgu = 2 D + pad_gu); u_shift: floats the [U | V] view starts
    into its buffer (1: a base address that is no multiple of 16).  expect: dict(fwd=, bwd=, second=, vec=[, nb_fwd=, nb_bwd=]) with the
    names of functional.GR_FIRST / GR_SECOND - asserted against functional.gr_plan BEFORE anything is launched."""
    N, E, D = L.N, L.E, T * F
    aggr, scal = tuple(GR_AGGR[a] for a in aggs), tuple(GR_SCALER[s] for s in scalers)
    K, S = len(aggr), len(scal)
    given = inputs is not None
    if graph is None:
        graph = Fn.GRGraph(torch.from_numpy(L.edge_index()).to(DEV), N)
    csr = graph.by_target
    long_nodes = csr.long_nodes if with_list else None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    Ud = Vd = Zd = zd = ind = None
    if given:
        ind = t(inputs.reshape(E, D))
    else:
        _, UV = _padded(N, 2 * D, pad_uv, shift=u_shift)
        UV[:, :D] = t(U); UV[:, D:] = t(V)
        Ud, Vd = UV[:, :D], UV[:, D:]
        if Z is not None:
            rows = Z if zidx is not None or not by_pos else Z[L.perm]
            _, Zd = _padded(len(rows), D, pad_z)
            Zd.copy_(t(rows))
            if zidx is not None:
                zd = t((zidx[L.perm] if by_pos else zidx).astype(np.uint8))
    ldsave = D + pad_save
    side = int(Fn._lib.lib().mma_gr_arg_side_rows(E))
    amin = torch.full((N, ldsave), SENT8, dtype=torch.uint8, device=DEV) if 2 in aggr else None
    amax = torch.full((N, ldsave), SENT8, dtype=torch.uint8, device=DEV) if 3 in aggr else None
    amin_s = torch.full((side, ldsave), SENT32, dtype=torch.int32, device=DEV) if amin is not None else None
    amax_s = torch.full((side, ldsave), SENT32, dtype=torch.int32, device=DEV) if amax is not None else None
    stats = 4 in aggr or 5 in aggr
    mean = torch.full((N, ldsave), float("nan"), device=DEV) if stats else None
    var = torch.full((N, ldsave), float("nan"), device=DEV) if stats else None
    out = torch.full((N, T, S * K * F), float("nan"), device=DEV)
    drop = Fn.DropoutSpec(p, seed=seed)
    _, gmsg = _padded(max(E, 1), D, pad_g)
    gbuf, gUV = (None, None) if given else _padded(N, 2 * D, pad_gu)
    gU = None if given else gUV[:, :D]
    saved_any = amin is not None or amax is not None or stats

    def aligned(*ts):
        return all(x is None or x.data_ptr() % 16 == 0 for x in ts)

    common = dict(lduv=0 if given else Ud.stride(0), ldz=Zd.stride(0) if Zd is not None else 0, ldi=D if given else 0,
                  has_z=Zd is not None, given=given, has_stats=stats, has_list=with_list, drop_on=p > 0)
    saved = (amin, amax, amin_s, amax_s, mean, var)
    plan_f = Fn.gr_plan(N, E, T, F, aggr, scal, ldsave=ldsave if saved_any else 0,
                        aligned=aligned(out, ind, Ud, Vd, Zd, *saved), **common)
    plan_b = Fn.gr_plan(N, E, T, F, aggr, scal, backward=True, ldsave=ldsave if saved_any else 0, ldg=gmsg.stride(0),
                        ldgu=0 if given else gUV.stride(0), aligned=aligned(gmsg, gU, ind, Ud, Vd, Zd, *saved), **common)
    if expect is not None:
        got = dict(fwd=Fn.GR_FIRST[plan_f.first], bwd=Fn.GR_FIRST[plan_b.first], second=Fn.GR_SECOND[plan_f.second], vec=plan_f.vec)
        for key in ("nb_fwd", "nb_bwd"):
            if key in expect:
                got[key] = (plan_f if key == "nb_fwd" else plan_b).nb
        assert got == expect, "the case names %s, the ladder plans %s (forward %s, backward %s)" % (expect, got, plan_f, plan_b)
        assert plan_b.second == plan_f.second and plan_b.vec == plan_f.vec, (plan_f, plan_b)
    r = Result()
    r.plan_f, r.plan_b, r.graph = plan_f, plan_b, graph
    Fn._gr_call("mma_gr_fused_fwd", csr, Ud, Vd, Zd, by_pos, ind,
                (ptr(out), ptr(amin), ptr(amax), ptr(amin_s), ptr(amax_s), ptr(mean), ptr(var), ldsave, ptr(long_nodes)),
                N, E, T, F, aggr, scal, AVG["log"], AVG["lin"], drop, zd)
    r.gmsg, r.gU, r.gmsg_pad, r.gu_pad, r.rm_msg, r.rm_u = [], [], [], [], [], []
    for g in gouts:
        gmsg.fill_(float("nan"))
        if gbuf is not None:
            gbuf.fill_(float("nan"))
        rm = torch.zeros(E + N, device=DEV) if row_max else None
        Fn._gr_call("mma_gr_fused_bwd", csr, Ud, Vd, Zd, by_pos, ind,
                    (ptr(t(g)), ptr(amin), ptr(amax), ptr(amin_s), ptr(amax_s), ptr(mean), ptr(var), ldsave, ptr(long_nodes), ptr(gmsg),
                     gmsg.stride(0), ptr(gU), 0 if given else gUV.stride(0), ptr(rm[:E]) if row_max else None,
                     ptr(rm[E:]) if row_max else None),
                    N, E, T, F, aggr, scal, AVG["log"], AVG["lin"], drop, zd)
        torch.cuda.synchronize()
        gm = gmsg[:E].cpu().numpy()
        r.gmsg.append(gm)                                            # rows by position with by_pos, else by original id
        r.gU.append(None if given else gU.cpu().numpy())
        # the pitch columns behind the rows: [U | V]'s right half is the caller's (the dV segment sum), so it counts as padding here
        r.gmsg_pad.append(gmsg.as_strided((max(E, 1), pad_g), (D + pad_g, 1), D).cpu().numpy() if pad_g else None)
        r.gu_pad.append(None if given else gUV.as_strided((N, D + pad_gu), (2 * D + pad_gu, 1), D).cpu().numpy())
        if row_max:
            r.rm_msg.append(rm[:E].cpu().numpy()); r.rm_u.append(rm[E:].cpu().numpy())
    torch.cuda.synchronize()
    csr.check()
    r.out = out.cpu()
    r.amin = amin.cpu().numpy() if amin is not None else None
    r.amax = amax.cpu().numpy() if amax is not None else None
    r.amin_side = amin_s.cpu().numpy() if amin_s is not None else None
    r.amax_side = amax_s.cpu().numpy() if amax_s is not None else None
    return r


def assert_saved_args(L, D, a8, side, want, what):
    """The saved arg of every (node, column): the byte for segments below 256 edges, the int32 row ceil(rowptr[n] / 256) of the side
    table for the others; every side row that belongs to no such segment still holds SENT32, and so do the pitch columns."""
    long = np.nonzero(L.deg >= 256)[0]
    short = np.nonzero((L.deg > 0) & (L.deg < 256))[0]
    assert np.array_equal(a8[short, :D].astype(np.int64), want[short]), what + ": arg bytes differ from the oracle's offsets"
    rows = (L.rowptr[long] + 255) // 256
    assert len(set(rows.tolist())) == len(rows), what + ": two long segments share a side row"
    assert np.array_equal(side[rows, :D].astype(np.int64), want[long]), what + ": side-table rows differ from the oracle's offsets"
    others = np.setdiff1d(np.arange(side.shape[0]), rows)
    assert (side[others] == SENT32).all(), what + ": a side-table row of no long segment was written"
    assert (side[:, D:] == SENT32).all() and (a8[:, D:] == SENT8).all(), what + ": pitch columns of the saved args were written"
