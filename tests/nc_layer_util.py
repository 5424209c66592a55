"""What the GPU tests of the NC layer's newer kernels share (tests/test_nc_std_gpu.py, test_nc_bf16_gpu.py, test_nc_std_bf16_gpu.py,
test_nc_halo_gpu.py):
the graphs, the plain torch statement of the `std` aggregator, the layer constructor and the std run.  Each graph is built once, here.

Shapes are the smallest at which the kernels take another path: degrees around the group / wavefront item split and the 64-index
chunk, a hub cut into partial slots (forward and transposed).  Where the three files want different defaults (fp32 or bf16 tables,
weights as drawn or on the 2^-9 grid) each binds its own with functools.partial."""
import numpy as np
import torch

from golden.inputs import ALL_MASK_NAMES

DEV = "cuda:0"
C_OUT = 4
BF16 = torch.bfloat16


# ---- the definition, in torch (any dtype, CPU) ---------------------------------------------------------------------------------
def csr_of(add_all):
    deg = np.array([len(a) for a in add_all], dtype=np.int64)
    col = np.concatenate([np.asarray(a, dtype=np.int64) for a in add_all]) if deg.sum() else np.zeros(0, np.int64)
    return deg, col


def rounded(t, table_dtype):
    """The stored table: t rounded to bf16 and widened again; the gradient passes straight through (r - t is exact, t + (r - t) = r)."""
    if table_dtype == torch.float32:
        return t
    r = t.detach().to(torch.bfloat16).to(t.dtype)
    return t + (r - t.detach())


def std_oracle(x, W, add_all, activation, keep=None, p=0.0, table_dtype=torch.float32):
    """m (N,H) = sqrt(relu(msq - mean^2) + 1e-5) of the masked neighbour messages; keep: (E,H) 0/1 or None; table_dtype: what P and Q
    are stored as (bf16: rounded before z = P[dst] + Q[col])."""
    N, H = x.shape
    deg, col = csr_of(add_all)
    dst = torch.from_numpy(np.repeat(np.arange(N), deg))
    col = torch.from_numpy(col)
    P, Q = rounded(x @ W[:H], table_dtype), rounded(x @ W[H:], table_dtype)
    z = P[dst] + Q[col]
    a = z if activation == "new_sigmoid" else torch.sigmoid(z)
    mu = a * x[col]
    if keep is not None:
        mu = (keep.to(x.dtype) / (1.0 - p)) * mu
    d = torch.from_numpy(np.maximum(deg, 1)).to(x.dtype).unsqueeze(1)
    mean = torch.zeros(N, H, dtype=x.dtype).index_add(0, dst, mu) / d
    msq = torch.zeros(N, H, dtype=x.dtype).index_add(0, dst, mu * mu) / d
    return torch.sqrt(torch.relu(msq - mean * mean) + 1e-5)


def oracle_with_grads(x, W, add_all, activation, cot, keep=None, p=0.0, dtype=torch.float64, table_dtype=torch.float32):
    """(m, gx, gmask_std) of std_oracle in `dtype`, the gradients those of <m, cot>."""
    xo = x.to(dtype).requires_grad_(True)
    Wo = W.to(dtype).requires_grad_(True)
    m = std_oracle(xo, Wo, add_all, activation, keep, p, table_dtype)
    gx, gW = torch.autograd.grad((m * cot.to(dtype)).sum(), [xo, Wo])
    return m.detach().numpy(), gx.numpy(), gW.numpy()


# ---- graphs --------------------------------------------------------------------------------------------------------------------
BOUNDARY_DEGREES = [0, 1, 2, 7, 8, 9, 63, 64, 65]      # MMA_SMALL_GROUP = 8: group / wavefront items; 64: one index chunk of a wavefront


def boundary_graph():
    """N = 120.  Targets 0..8 have the boundary in-degrees (distinct sources), sources 10..18 the same OUT-degrees (distinct targets
    among 20..119): the transposed lists meet the same boundaries.  The other targets get 0..5 random neighbours."""
    rng = np.random.default_rng(7)
    N = 120
    edges = set()
    for t, d in enumerate(BOUNDARY_DEGREES):
        for s in rng.choice(np.arange(19, N), size=d, replace=False):
            edges.add((t, int(s)))
    for k, d in enumerate(BOUNDARY_DEGREES):
        for t in rng.choice(np.arange(20, N), size=d, replace=False):
            edges.add((int(t), 10 + k))
    for t in range(20, N):
        for s in rng.choice(np.arange(19, N), size=rng.integers(0, 6), replace=False):
            edges.add((t, int(s)))
    add_all = [sorted(s for (t, s) in edges if t == i) for i in range(N)]
    assert [len(add_all[t]) for t in range(9)] == BOUNDARY_DEGREES
    return add_all


def hub_graph():
    """N = 300: target 0 has 200 distinct neighbours, source 1 has 200 out-edges; everything else 0..4 neighbours."""
    rng = np.random.default_rng(11)
    N = 300
    edges = {(0, s) for s in range(60, 260)} | {(t, 1) for t in range(80, 280)}
    for t in range(2, N):
        for s in rng.choice(np.arange(2, N), size=rng.integers(0, 5), replace=False):
            edges.add((t, int(s)))
    return [sorted(s for (t, s) in edges if t == i) for i in range(N)]


def small_graph(N=150, seed=9):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(N, size=rng.integers(0, 8), replace=False).tolist()) for _ in range(N)]


def halo_graph():
    """(add_all, S): the halo form of one shard - N = 150 targets (rows 0..149) over S = 300 source rows, rows 150..299 sources only.
    Target 0 is a hub over own AND halo sources; targets 1..9 have the boundary in-degrees from halo sources alone; own source 10 and
    halo source 290 have 100 out-edges each; halo sources 291..299 the boundary OUT-degrees; the other targets 2..6 more sources.  Some
    own sources and halo source 291 have no out-edge at all."""
    rng = np.random.default_rng(13)
    N, S = 150, 300
    edges = {(0, s) for s in range(60, 260)}
    for k, d in enumerate(BOUNDARY_DEGREES):
        for s in rng.choice(np.arange(150, 290), size=d, replace=False):
            edges.add((1 + k, int(s)))
    edges |= {(t, 10) for t in range(20, 120)} | {(t, 290) for t in range(30, 130)}
    for k, d in enumerate(BOUNDARY_DEGREES):
        for t in rng.choice(np.arange(20, 150), size=d, replace=False):
            edges.add((int(t), 291 + k))
    for t in range(10, N):
        for s in rng.choice(np.arange(11, 290), size=rng.integers(2, 7), replace=False):
            edges.add((t, int(s)))
    return [sorted(s for (t, s) in edges if t == i) for i in range(N)], S


def embed(add_all, S):
    """The halo problem as an ordinary S-node graph: rows >= N take no in-edge (and, in the tests, a zero cotangent).  The oracles take
    it unchanged with x of S rows; their m[:N], their full-S gx and their mask-weight gradients are the halo form's values."""
    return add_all + [[]] * (S - len(add_all))


BOUNDARY = boundary_graph()
HUB = hub_graph()
SMALL = small_graph()


def small_graph_with_a_hub():
    """SMALL plus one target with 40 neighbours and one source with 40 out-edges: items per wavefront, items per lane group and, with
    chunk=32, one hub in two partial slots each way - the plan the one-launch form takes with its ticket counter."""
    add_all = [list(a) for a in SMALL]
    add_all[0] = list(range(10, 50))
    for t in range(60, 100):
        add_all[t] = sorted(set(add_all[t]) | {1})
    return add_all


def normalized_adj(add_all):
    """D^-1 (A + I), the adjacency the reference's training script hands to forward (utils.py normalize): dense float64 and sparse."""
    N = len(add_all)
    A = np.eye(N)
    for i, a in enumerate(add_all):
        A[i, a] = 1.0
    A /= A.sum(1, keepdims=True)
    idx = np.nonzero(A)
    sp = torch.sparse_coo_tensor(torch.from_numpy(np.stack(idx)), torch.from_numpy(A[idx].astype(np.float32)), (N, N))
    return torch.from_numpy(A), sp.to(DEV)


def degenerate_targets(add_all):
    """Targets whose exact variance is 0 by construction: degree 0, degree 1, all edges from one source."""
    return [i for i, a in enumerate(add_all) if len(a) <= 1 or len(set(a)) == 1]


# ---- the layer -------------------------------------------------------------------------------------------------------------------
def make_layer(add_all, H, aggs, activation="sigmoid", p=0.0, chunk=None, seed=0, grid=False, scale=1.0, **kw):
    """mma_amd.MMA with every mask weight drawn from `seed`; kw (logit_dtype, strict_reference, ...) goes to the layer as given, so what
    is not named keeps the layer's own default.  grid: the weights rounded to multiples of 2^-9, times `scale` (a power of two) - the
    grid on which the bf16 files' P and Q are exact (their module docstrings)."""
    import mma_amd
    assert grid or scale == 1.0
    torch.manual_seed(seed)
    P = lambda *s: torch.nn.Parameter(torch.empty(*s, device=DEV))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    if chunk is not None:
        kw["chunk"] = chunk
    layer = mma_amd.MMA(add_all, activation, 2, H, C_OUT, P(H, C_OUT), P(C_OUT), *masks, p, list(aggs), DEV, **kw)     # reset_parameters draws
    if grid:
        with torch.no_grad():
            for w in masks:
                w.copy_(torch.round(w * 512.0) / 512.0 * scale)
    return layer


def std_inputs(add_all, H, seed=3, x_grid=False):
    """x (N,H) uniform in [-1, 1] - x_grid: in multiples of 2^-5 - and a cotangent for m."""
    rng = np.random.default_rng(seed)
    N = len(add_all)
    if x_grid:
        x = torch.from_numpy((rng.integers(-32, 33, (N, H)) / 32.0).astype(np.float32))
    else:
        x = torch.from_numpy(rng.uniform(-1, 1, (N, H)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
    # exact variance 0: relu' decides the gradient there; checked by construction (test_nc_std_gpu.py: test_degenerate_variance), not by parity
    cot[degenerate_targets(add_all)] = 0
    return x, cot


def run_std(layer, x, cot):
    """(m, gx, gmask_std) of layer.learnable_std on the GPU."""
    xg = x.to(DEV).requires_grad_(True)
    layer.mask_std.grad = None
    m = layer.learnable_std(xg, None)
    gx, gw = torch.autograd.grad((m * cot.to(DEV)).sum(), [xg, layer.mask_std])
    torch.cuda.synchronize()
    return m.detach(), gx, gw
