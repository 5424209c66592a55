"""GPU tests of the bf16 logit tables of the `std` aggregator (MMA(..., strict_reference=False, logit_dtype=torch.bfloat16);
include/mma_amd.h ABI 40: mma_nc_std_fwd_h / mma_nc_std_bwd_h, csrc/nc_moments.hip) against the plain torch statement of the aggregator
(tests/nc_layer_util.py: std_oracle) in which P and Q are rounded with .to(torch.bfloat16).to(dtype) before z = P[dst] + Q[col].
float64 on the CPU is the truth, the same statement in float32 the reference value, and the bar is the project's own, unchanged
(golden_util.check_close with truth).

As in tests/test_nc_bf16_gpu.py the rounding has to be the SAME on the three sides, so the inputs sit on grids on which P = x W[:H] and
Q = x W[H:] are exact in every arithmetic that takes part: x in multiples of 2^-5 within [-1, 1], the mask weights in multiples of 2^-9
within +-1/sqrt(H) - a sum of H <= 128 products is a multiple of 2^-14 below 2^6, at most 20 bits: exact in float32 under any summation
order and in the split-fp16 GEMMs.  The layer test asserts it (the saved bf16 table equals the oracle's bit for bit).  The gradient
passes the rounding straight through, on both sides.

Graphs and shapes are those of tests/test_nc_std_gpu.py (tests/nc_layer_util.py): degrees around the group / wavefront item split and
the 64-index chunk, a hub cut into partial slots both ways, H = 8 / 20 / 128 (8-byte table vectors; 20: a partial lane group) and H = 6 (scalar
2-byte loads).  This file's own defaults: bf16 tables, the weights on the 2^-9 grid, x on the 2^-5 grid."""
import functools

import numpy as np
import pytest
import torch

from golden_util import check_close
from golden.inputs import ALL_MASK_NAMES
from nc_layer_util import BF16, BOUNDARY as _BOUNDARY, C_OUT, DEV, HUB as _HUB, SMALL as _SMALL, csr_of, normalized_adj, rounded, run_std
import nc_layer_util
from oracle import nc_oracle as O

pytestmark = pytest.mark.gpu
F32 = torch.float32
std_oracle = functools.partial(nc_layer_util.std_oracle, table_dtype=BF16)
oracle_with_grads = functools.partial(nc_layer_util.oracle_with_grads, table_dtype=BF16)
make_layer = functools.partial(nc_layer_util.make_layer, logit_dtype=BF16, strict_reference=False, grid=True)
inputs = functools.partial(nc_layer_util.std_inputs, x_grid=True)
_ORACLE = {}


def oracles(key, x, W, add_all, activation, cot, keep=None, p=0.0, table_dtype=BF16):
    """(float32 reference, float64 truth) of (m, gx, gmask_std), computed once per `key` and shared by the tests that need them."""
    if key not in _ORACLE:
        _ORACLE[key] = tuple(oracle_with_grads(x, W, add_all, activation, cot, keep, p, dt, table_dtype=table_dtype) for dt in (torch.float32, torch.float64))
    return _ORACLE[key]


def compare(got, want, truth, what, names=("m", "gx", "gmask_std")):
    for g, w, t, name in zip(got, want, truth, names):
        err = np.abs(g.detach().cpu().numpy().astype(np.float64) - t)
        print("%s/%s: max |got - fp64| %.3g, max |fp32 ref - fp64| %.3g" % (what, name, err.max(), np.abs(w.astype(np.float64) - t).max()))
        check_close(g, w, None, None, what=what + "/" + name, signed_sum=True, truth=t)


# ---- 1: item boundaries x widths x activations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["sigmoid", "new_sigmoid"])
@pytest.mark.parametrize("H", [8, 20, 128, 6])           # 6: scalar 2-byte loads; 20: 8-byte vectors with a partial lane group
def test_item_boundaries(H, activation):
    layer = make_layer(_BOUNDARY, H, ["std"], activation, chunk=512)        # chunk > 65: every segment is one item
    g = layer.graph(torch.device(DEV))
    assert g.n_slots == 0 and g.t_n_slots == 0
    x, cot = inputs(_BOUNDARY, H)
    got = run_std(layer, x, cot)
    want, truth = oracles(("boundary", H, activation), x, layer.mask_std.detach().cpu(), _BOUNDARY, activation, cot)
    compare(got, want, truth, "std-bf16/boundary/H%d/%s" % (H, activation))


# ---- 2: a hub in partial slots, forward and transposed -------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 6])
def test_hub_chunks(H):
    x, cot = inputs(_HUB, H)
    small = make_layer(_HUB, H, ["std"], chunk=32)
    whole = make_layer(_HUB, H, ["std"], chunk=512)           # same seed: same weights
    assert torch.equal(small.mask_std, whole.mask_std)
    g = small.graph(torch.device(DEV))
    assert g.n_slots == 7 and g.hubs.cpu()[:, 0].tolist() == [0] and g.t_n_slots == 7 and g.t_hubs.cpu()[:, 0].tolist() == [1]
    assert whole.graph(torch.device(DEV)).n_slots == 0
    a, b, w = run_std(small, x, cot), run_std(small, x, cot), run_std(whole, x, cot)
    for u, v in zip(a, b):
        assert torch.equal(u, v)                                # fixed slot order, no atomics: bit-equal runs
    want, truth = oracles(("hub", H), x, small.mask_std.detach().cpu(), _HUB, "sigmoid", cot)
    compare(a, want, truth, "std-bf16/hub/H%d/chunk32" % H)
    compare(w, want, truth, "std-bf16/hub/H%d/whole" % H)
    compare(a, [t.cpu().numpy() for t in w], truth, "std-bf16/hub/H%d/chunk32-vs-whole" % H)


# ---- 3: dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,graph,chunk", [(20, "boundary", 512), (128, "hub", 32), (6, "hub", 32)])
def test_explicit_keep_mask(H, graph, chunk):
    from mma_amd import functional as Fn
    add_all = _BOUNDARY if graph == "boundary" else _HUB
    E = sum(len(a) for a in add_all)
    keep = torch.from_numpy((np.random.default_rng(5).random((1, E, H)) >= 0.5).astype(np.uint8))
    layer = make_layer(add_all, H, ["std"], "sigmoid", 0.5, chunk=chunk)
    layer.drop_override = Fn.DropoutSpec(0.5, keep=keep.to(DEV))
    x, cot = inputs(add_all, H)
    got = run_std(layer, x, cot)
    want, truth = oracles(("keep", graph, H), x, layer.mask_std.detach().cpu(), add_all, "sigmoid", cot, keep=keep[0], p=0.5)
    compare(got, want, truth, "std-bf16/keep/%s/H%d" % (graph, H))


@pytest.mark.parametrize("H,p", [(128, 0.5), (6, 0.5), (20, 0.3)])            # 0.3: a threshold that is no multiple of 256 (16-bit form)
def test_hash_dropout_is_repeatable_and_seeded(H, p):
    from mma_amd import functional as Fn
    layer = make_layer(_HUB, H, ["std"], "sigmoid", p, chunk=32)
    x, cot = inputs(_HUB, H)
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDEF)
    a, b = run_std(layer, x, cot), run_std(layer, x, cot)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDF0)
    c = run_std(layer, x, cot)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    layer.drop_override = Fn.DropoutSpec(0.0)
    assert not torch.equal(a[0], run_std(layer, x, cot)[0])


# ---- 4: the same function as the fp32 kernels, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,graph,chunk,p", [(20, "boundary", 512, 0.5), (6, "boundary", 512, 0.3), (128, "hub", 32, 0.5)])
def test_bf16_tables_give_the_fp32_kernels_results_on_representable_values(H, graph, chunk, p):
    """fp32 leaf tables whose values are bf16 numbers already: the conversion is exact, the kernels' widening is exact, so the two
    table types must give the same bits in m, gx, gP and gQ."""
    from mma_amd import functional as Fn
    from mma_amd.graph import NCGraph
    add_all = _BOUNDARY if graph == "boundary" else _HUB
    N = len(add_all)
    g = NCGraph.from_add_all(add_all, torch.device(DEV), chunk=chunk, H=H)
    assert (g.n_slots > 0) == (graph == "hub")
    x, cot = inputs(add_all, H)
    rng = np.random.default_rng(21)
    tables = [torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(BF16).to(F32) for _ in range(2)]
    drop = Fn.DropoutSpec(p, seed=0xC0FFEE)

    def run(**kw):
        xg = x.to(DEV).requires_grad_(True)
        P, Q = (t.to(DEV).requires_grad_(True) for t in tables)
        m = Fn.nc_std_aggregate(xg, P, Q, g, Fn.ACT_SIGMOID, drop, **kw)
        grads = torch.autograd.grad((m * cot.to(DEV)).sum(), [xg, P, Q])
        assert all(t.dtype == F32 for t in grads)              # gP / gQ come back in fp32 (straight-through)
        torch.cuda.synchronize()
        return (m.detach(),) + grads

    full, half = run(), run(logit_dtype=BF16)
    for u, v, name in zip(full, half, ("m", "gx", "gP", "gQ")):
        assert bool(torch.isfinite(u).all()) and float(u.abs().max()) > 0, name
        assert torch.equal(u, v), "%s differs between fp32 and bf16 tables (max |diff| %.3g)" % (name, float((u - v).abs().max()))
    # bf16 tables given as such: the same bits again
    xg = x.to(DEV)
    with torch.no_grad():
        m_h = Fn.nc_std_aggregate(xg, tables[0].to(DEV).to(BF16), tables[1].to(DEV).to(BF16), g, Fn.ACT_SIGMOID, drop)
    assert torch.equal(m_h, full[0])


# ---- 5: large logits show the rounding ----------------------------------------------------------------------------------------------------
def test_large_logits_show_the_rounding_and_match_the_bf16_oracle():
    """Mask weights scaled by 16, raw logits: |z| reaches 8 and beyond, a bf16 step there is 2^-5.  The bf16 layer's learnable_std then
    differs from the fp32 layer's by more than the bar allows - and still meets that bar against the oracle that rounds the same tables."""
    H = 20
    half = make_layer(_SMALL, H, ["std"], "new_sigmoid", scale=16.0)
    full = make_layer(_SMALL, H, ["std"], "new_sigmoid", scale=16.0, logit_dtype=F32)
    assert torch.equal(half.mask_std, full.mask_std)
    x, cot = inputs(_SMALL, H)
    W = half.mask_std.detach().cpu()
    z_max = float((x @ W[:H]).abs().max() + (x @ W[H:]).abs().max())
    assert z_max >= 8.0, z_max
    got_h, got_f = run_std(half, x, cot), run_std(full, x, cot)
    want, truth = oracles(("large", "bf16"), x, W, _SMALL, "new_sigmoid", cot)
    compare(got_h, want, truth, "std-bf16/large-logits")
    w32, t32 = oracles(("large", "fp32"), x, W, _SMALL, "new_sigmoid", cot, table_dtype=F32)
    compare(got_f[:1], w32, t32, "std-fp32/large-logits")
    with pytest.raises(AssertionError, match="outside"):
        compare(got_h[:1], w32, t32, "std-bf16-vs-fp32-oracle/large-logits")
    diff = (got_h[0] - got_f[0]).abs().max().item()
    print("large logits: max |z| %.3g, max |m(bf16) - m(fp32)| %.3g" % (z_max, diff))
    assert diff > 1e-3


# ---- 6: through the layer ------------------------------------------------------------------------------------------------------------
MIXED = ["sum", "mean3", "std", "max"]


def autograd_nodes(out):
    seen, todo = [], [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.append(fn)
        todo += [f for f, _ in fn.next_functions]
    return seen


def layer_oracle(layer, names, x, add_all, A64, cot, dtype, activation="sigmoid"):
    """A (c (msum W)) + b with msum = the fused masks' sum + m_std, and its gradients with respect to x, the mask weights, W and b."""
    N, H = x.shape
    deg, col = csr_of(add_all)
    dst, col = torch.from_numpy(np.repeat(np.arange(N), deg)), torch.from_numpy(col)
    d = torch.from_numpy(np.maximum(deg, 1)).to(dtype).unsqueeze(1)
    factor = layer._scaler_factor(N, torch.device(DEV)).detach().cpu().reshape(-1, 1).to(dtype)
    xo = x.to(dtype).requires_grad_(True)
    leaves = [getattr(layer, "mask_" + n).detach().cpu().to(dtype).requires_grad_(True) for n in names]
    leaves += [layer.weight.detach().cpu().to(dtype).requires_grad_(True), layer.bias.detach().cpu().to(dtype).requires_grad_(True)]
    msum = 0
    for name, W in zip(names, leaves):
        if name == "std":
            msum = msum + std_oracle(xo, W, add_all, activation)
            continue
        P, Q = rounded(xo @ W[:H], BF16), rounded(xo @ W[H:], BF16)
        z = P[dst] + Q[col]
        a = z if O.uses_raw_logits(name, activation) else torch.sigmoid(z)
        s = torch.zeros(N, H, dtype=dtype).index_add(0, dst, a * xo[col])
        msum = msum + O._combine(O.AGGREGATORS[name][0], xo, s, d)
    out = A64.to(dtype) @ (factor * (msum @ leaves[-2])) + leaves[-1]
    grads = torch.autograd.grad((out * cot.to(dtype)).sum(), [xo] + leaves)
    return [out.detach().numpy()] + [g.numpy() for g in grads]


def test_layer_with_a_mixed_aggregator_list():
    H, names = 20, MIXED
    N = len(_SMALL)
    A64, adj = normalized_adj(_SMALL)
    layer = make_layer(_SMALL, H, names, "sigmoid", 0.0)
    x, _ = inputs(_SMALL, H)
    cot = torch.from_numpy(np.random.default_rng(8).standard_normal((N, C_OUT)).astype(np.float32))
    xg = x.to(DEV).requires_grad_(True)
    params = [getattr(layer, "mask_" + n) for n in names] + [layer.weight, layer.bias]
    out = layer(xg, adj)
    # the std node: its saved [P | Q] is bf16, and it keeps no fp32 (N,H) or (N,2H) table (x and the (N,3H) moment rows are not tables)
    std_nodes = [fn for fn in autograd_nodes(out) if "NCStd" in type(fn).__name__]
    assert len(std_nodes) == 1
    saved = [t for t in std_nodes[0].saved_tensors if t is not None]
    tables = [t for t in saved if t.dtype == BF16]
    assert len(tables) == 1 and tables[0].shape == (N, 2 * H)
    f32_rows = [t for t in saved if t.dtype == F32 and t.shape[0] == N and t is not saved[0]]
    assert saved[0].shape == (N, H) and torch.equal(saved[0], xg.detach())                       # x itself
    assert all(tuple(t.shape) not in ((N, H), (N, 2 * H)) for t in f32_rows), [tuple(t.shape) for t in f32_rows]
    # no fp32 (N,H) / (N,2H) logit table anywhere else in the graph either: every mask's P and Q are bf16
    W = layer.mask_std.detach().cpu()
    pq = torch.cat([x @ W[:H], x @ W[H:]], 1)
    assert torch.equal(tables[0].cpu().view(torch.int16), pq.to(BF16).view(torch.int16))         # the grids make the forward GEMM exact
    assert torch.equal(pq.double(), torch.cat([x.double() @ W[:H].double(), x.double() @ W[H:].double()], 1))
    grads = torch.autograd.grad((out * cot.to(DEV)).sum(), [xg] + params)
    want = layer_oracle(layer, names, x, _SMALL, A64, cot, torch.float32)
    truth = layer_oracle(layer, names, x, _SMALL, A64, cot, torch.float64)
    tags = ["out", "gx"] + ["gmask[%s]" % n for n in names] + ["gweight", "gbias"]
    for g, w, t, tag in zip([out.detach()] + list(grads), want, truth, tags):
        if tag == "gbias":
            g, w, t = g.reshape(1, -1), w.reshape(1, -1), t.reshape(1, -1)
        print("std-bf16/layer/%s: max |got - fp64| %.3g" % (tag, np.abs(g.detach().cpu().numpy() - t).max()))
        check_close(g, w, None, None, what="std-bf16/layer/" + tag, signed_sum=True, truth=t)


def test_float32_keyword_equals_no_keyword_bit_for_bit():
    import mma_amd
    H, names = 20, MIXED
    _, adj = normalized_adj(_HUB)
    x, _ = inputs(_HUB, H)
    cot = torch.from_numpy(np.random.default_rng(8).standard_normal((len(_HUB), C_OUT)).astype(np.float32)).to(DEV)
    explicit = make_layer(_HUB, H, names, "sigmoid", chunk=32, logit_dtype=F32)
    torch.manual_seed(0)
    P = lambda *s: torch.nn.Parameter(torch.empty(*s, device=DEV))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    plain = mma_amd.MMA(_HUB, "sigmoid", 2, H, C_OUT, P(H, C_OUT), P(C_OUT), *masks, 0.0, list(names), DEV, chunk=32,
                        strict_reference=False)                                                    # no logit_dtype keyword
    with torch.no_grad():
        for n in ALL_MASK_NAMES:
            getattr(plain, "mask_" + n).copy_(getattr(explicit, "mask_" + n))
        plain.weight.copy_(explicit.weight); plain.bias.copy_(explicit.bias)
    assert plain.logit_dtype == F32

    def run(layer):
        xg = x.to(DEV).requires_grad_(True)
        out = layer(xg, adj)
        assert not any(t.dtype == BF16 for fn in autograd_nodes(out) for t in getattr(fn, "saved_tensors", ()) if t is not None)
        params = [getattr(layer, "mask_" + n) for n in names] + [layer.weight, layer.bias]
        return [out.detach()] + list(torch.autograd.grad((out * cot).sum(), [xg] + params))

    for u, v in zip(run(explicit), run(plain)):
        assert torch.equal(u, v)


# ---- 7: graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_with_fresh_std_dropout_bits():
    H = 20
    _, adj = normalized_adj(_SMALL)
    layer = make_layer(_SMALL, H, ["mean", "std"], "sigmoid", 0.5)
    layer.graph_capturable = True
    x = inputs(_SMALL, H)[0].to(DEV).requires_grad_(True)
    cot = torch.randn(len(_SMALL), C_OUT, device=DEV)

    def step():
        x.grad = None
        out = layer(x, adj)
        out.backward(cot)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                       # warm-up: the seed states are drawn, the plans and caches built
            step()
    torch.cuda.current_stream().wait_stream(s)
    assert layer._seeds.n == 2                   # one device seed for the fused group, one for std
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_static = step()
    outs, seeds = [], []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        outs.append((out_static.clone(), x.grad.clone()))
        seeds.append(layer._seed_buf.cpu().tolist())
    assert seeds[0][1] != seeds[1][1] and seeds[0][0] != seeds[0][1]
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)
