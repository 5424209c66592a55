"""GPU tests of the bf16 logit tables of the fused NC kernels (MMA(..., logit_dtype=torch.bfloat16); include/mma_amd.h ABI 38:
mma_nc_fused_fwd_h / mma_nc_fused_bwd_h / mma_rows_to_bf16) against a plain torch restatement of the fused aggregators in which P and
Q are rounded with .to(torch.bfloat16).to(dtype) before z = P[dst] + Q[col].  float64 on the CPU is the truth, the same statement in
float32 the reference value, and the bar is the project's own, unchanged (golden_util.check_close with truth).

The rounding has to be the SAME on the three sides (float64, float32, GPU), else one logit that sits at a bf16 rounding boundary moves
by 2^-9 of its size - a hundred times the bar - although nothing is wrong.  So the inputs are drawn on grids on which P = x W[:H] and
Q = x W[H:] are exact in every arithmetic that takes part: x in multiples of 2^-5 within [-1, 1] (6 bits), the mask weights in multiples
of 2^-9 within +-1/sqrt(H) (8 bits at the smallest H, 6): a product has at most 14 bits, a sum of H <= 128 of them is a multiple of 2^-14
below 2^6, i.e. at most 20 bits - exact in float32 under any summation order, and exact in the split-fp16 GEMMs, whose pieces hold 11
bits.  The layer tests assert this (the saved bf16 table equals the oracle's bit for bit).  Only the tables are special: the bf16
rounding itself moves the logits by up to 2^-9 |z| ~ 1e-3, every sum runs over inexact fp32 terms, and the bar follows the data.
The gradient passes the rounding straight through, on both sides.

Shapes are the smallest at which the kernels take another path (the graphs of tests/nc_layer_util.py).  This file's own defaults: bf16
tables, the weights on the 2^-9 grid, x on the 2^-5 grid."""
import functools

import numpy as np
import pytest
import torch

from golden_util import check_close
from golden.inputs import ALL_MASK_NAMES
from nc_layer_util import (BF16, BOUNDARY as _BOUNDARY, C_OUT, DEV, HUB as _HUB, SMALL as _SMALL, csr_of, normalized_adj, rounded,
                           small_graph_with_a_hub)
import nc_layer_util
from oracle import nc_oracle as O

pytestmark = pytest.mark.gpu
FIVE = ["sum", "mean3", "max", "min", "softmax"]
EIGHT = ["sum", "mean", "max", "min", "softmax", "softmin", "sum2", "mean3"]
_SMALL_HUB = small_graph_with_a_hub()
make_layer = functools.partial(nc_layer_util.make_layer, logit_dtype=BF16, grid=True)


# ---- the definition, in torch (any dtype, CPU) ---------------------------------------------------------------------------------
def fused_oracle(x, Ws, names, add_all, activation, keeps=None, p=0.0, table_dtype=BF16):
    """m (K,N,H): the fused aggregators `names` with mask weights Ws[k] (2H,H); keeps: (K,E,H) 0/1 or None."""
    N, H = x.shape
    deg, col = csr_of(add_all)
    dst = torch.from_numpy(np.repeat(np.arange(N), deg))
    col = torch.from_numpy(col)
    d = torch.from_numpy(np.maximum(deg, 1)).to(x.dtype).unsqueeze(1)
    ms = []
    for k, name in enumerate(names):
        W = Ws[k]
        P, Q = rounded(x @ W[:H], table_dtype), rounded(x @ W[H:], table_dtype)
        z = P[dst] + Q[col]
        a = z if O.uses_raw_logits(name, activation) else torch.sigmoid(z)
        if keeps is not None:
            a = a * (keeps[k].to(x.dtype) / (1.0 - p))
        s = torch.zeros(N, H, dtype=x.dtype).index_add(0, dst, a * x[col])
        ms.append(O._combine(O.AGGREGATORS[name][0], x, s, d))
    return torch.stack(ms)


def oracle_with_grads(x, Ws, names, add_all, activation, cot, cot_k, keeps=None, p=0.0, dtype=torch.float64, table_dtype=BF16):
    """m (K,N,H), msum, and the gradients of <msum, cot> and of <m, cot_k> with respect to x and every mask weight."""
    xo = x.to(dtype).requires_grad_(True)
    Wo = [w.to(dtype).requires_grad_(True) for w in Ws]
    m = fused_oracle(xo, Wo, names, add_all, activation, keeps, p, table_dtype)
    gs = torch.autograd.grad((m.sum(0) * cot.to(dtype)).sum(), [xo] + Wo, retain_graph=True)
    gk = torch.autograd.grad((m * cot_k.to(dtype)).sum(), [xo] + Wo)
    n = lambda t: t.detach().numpy()
    return {"m": n(m), "msum": n(m.sum(0)), "gx": n(gs[0]), "gmask": [n(g) for g in gs[1:]], "gx_k": n(gk[0]), "gmask_k": [n(g) for g in gk[1:]]}


def inputs(add_all, H, K, seed=3):
    rng = np.random.default_rng(seed)
    N = len(add_all)
    x = torch.from_numpy((rng.integers(-32, 33, (N, H)) / 32.0).astype(np.float32))          # the 2^-5 grid
    cot = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32))
    cot_k = torch.from_numpy(rng.standard_normal((K, N, H)).astype(np.float32))
    return x, cot, cot_k


def weights(layer, names):
    return [getattr(layer, "mask_" + n) for n in names]


def run_layer(layer, names, x, cot, cot_k):
    """What oracle_with_grads returns, from the layer's two fused paths: reduce_k (the production path of forward()) and per mask."""
    Ws = weights(layer, names)
    xg = x.to(DEV).requires_grad_(True)
    msum = layer._aggregate_all(names, xg, reduce_k=True)
    gs = torch.autograd.grad((msum * cot.to(DEV)).sum(), [xg] + Ws)
    m = layer._aggregate_all(names, xg)
    gk = torch.autograd.grad((m * cot_k.to(DEV)).sum(), [xg] + Ws)
    torch.cuda.synchronize()
    return {"m": m.detach(), "msum": msum.detach(), "gx": gs[0], "gmask": list(gs[1:]), "gx_k": gk[0], "gmask_k": list(gk[1:])}


_ORACLE = {}


def oracles(key, x, layer, names, add_all, activation, cot, cot_k, keeps=None, p=0.0):
    """(float32 reference, float64 truth), computed once per `key` and shared by the tests that need them."""
    if key not in _ORACLE:
        Ws = [w.detach().cpu() for w in weights(layer, names)]
        _ORACLE[key] = tuple(oracle_with_grads(x, Ws, names, add_all, activation, cot, cot_k, keeps, p, dt) for dt in (torch.float32, torch.float64))
    return _ORACLE[key]


def compare(got, want, truth, names, what, parts=("m", "msum", "gx", "gmask", "gx_k", "gmask_k")):
    def one(g, w, t, tag):
        err = np.abs(g.detach().cpu().numpy().astype(np.float64) - t)
        print("%s/%s: max |got - fp64| %.3g, max |fp32 ref - fp64| %.3g" % (what, tag, np.nanmax(err), np.nanmax(np.abs(w.astype(np.float64) - t))))
        check_close(g, w, None, None, what=what + "/" + tag, signed_sum=True, truth=t)
    for part in parts:
        if part in ("gmask", "gmask_k"):
            for k, n in enumerate(names):
                one(got[part][k], want[part][k], truth[part][k], "%s[%s]" % (part, n))
        elif part == "m":
            for k, n in enumerate(names):
                one(got["m"][k], want["m"][k], truth["m"][k], "m[%s]" % n)
        else:
            one(got[part], want[part], truth[part], part)


def equal_runs(a, b):
    for key in a:
        for u, v in zip(a[key] if isinstance(a[key], list) else [a[key]], b[key] if isinstance(b[key], list) else [b[key]]):
            if not torch.equal(u, v):
                return False
    return True


# ---- the conversion kernel --------------------------------------------------------------------------------------------------------
def _special_values():
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    return np.concatenate([
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32),
        f([0x3F808000, 0x3F818000,            # ties: 1 + 2^-8 rounds DOWN to the even 0x3F80, 1 + 3 * 2^-8 rounds UP to the even 0x3F82
           0x3F808001, 0x3F807FFF,            # just above / below a tie
           0x3FFFFFFF, 0xBFFF8000,            # the mantissa carries into the exponent: -> 2.0, -2.0
           0x7F7FFFFF, 0xFF7FFFFF,            # the largest finite values round to +-inf
           0x7FC00001, 0xFFC00000, 0x7F800001])])   # NaNs of either sign, quiet and signalling


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(37, 20, 20, 20), (37, 20, 28, 24), (5, 6, 6, 6), (5, 6, 9, 7), (3, 8, 10, 8)])
def test_rows_to_bf16_equals_torch_bit_for_bit(rows, cols, ld_src, ld_dst):
    from mma_amd import functional as Fn
    rng = np.random.default_rng(rows * 100 + cols)
    a = (rng.standard_normal((rows, ld_src)) * np.exp(rng.uniform(-30, 30, (rows, ld_src)))).astype(np.float32)
    sp = _special_values()
    a.reshape(-1)[:min(sp.size, a.size)] = sp[:a.size]
    n_last = min(cols, sp.size)
    a[-1, :n_last] = sp[-n_last:]                               # the specials also in the last row, inside the converted columns
    src = torch.from_numpy(a).to(DEV)
    dst = torch.full((rows, ld_dst), 7.0, device=DEV, dtype=BF16)
    out = Fn.rows_to_bf16(src[:, :cols], dst[:, :cols])
    torch.cuda.synchronize()
    want = torch.from_numpy(a)[:, :cols].to(BF16).contiguous()  # torch's CPU conversion: round to nearest even
    assert int(torch.isnan(want).sum()) >= 3 and int(torch.isinf(want).sum()) >= 4
    assert bool((dst[:, cols:] == 7.0).all())                   # nothing written past the row
    for got in (out.cpu(), Fn.rows_to_bf16(src[:, :cols]).cpu()):          # the given (pitched) buffer, and one of its own
        # bit for bit, except the PATTERN of a NaN: torch itself writes 0x7FC0 from its scalar conversion and 0xFFFF from its vector
        # one (this comparison saw both), so a NaN is required to stay a NaN and every other element to have torch's bits
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
        assert bool((got.view(torch.int16)[nan] == 0x7FC0).all())


# ---- item boundaries x widths x activations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["sigmoid", "new_sigmoid"])
@pytest.mark.parametrize("H", [8, 20, 128, 6])           # 6: scalar 2-byte loads; 20: 8-byte vectors with a partial lane group
def test_item_boundaries(H, activation):
    layer = make_layer(_BOUNDARY, H, FIVE, activation, chunk=512)           # chunk > 65: every segment is one item
    g = layer.graph(torch.device(DEV))
    assert g.n_slots == 0 and g.t_n_slots == 0
    x, cot, cot_k = inputs(_BOUNDARY, H, len(FIVE))
    got = run_layer(layer, FIVE, x, cot, cot_k)
    want, truth = oracles(("boundary", H, activation), x, layer, FIVE, _BOUNDARY, activation, cot, cot_k)
    compare(got, want, truth, FIVE, "bf16/boundary/H%d/%s" % (H, activation))


# ---- a hub in partial slots, forward and transposed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [128, 6])
def test_hub_chunks(H):
    x, cot, cot_k = inputs(_HUB, H, len(FIVE))
    small = make_layer(_HUB, H, FIVE, chunk=32)
    whole = make_layer(_HUB, H, FIVE, chunk=512)              # same seed: same weights
    for a, b in zip(weights(small, FIVE), weights(whole, FIVE)):
        assert torch.equal(a, b)
    g = small.graph(torch.device(DEV))
    assert g.n_slots == 7 and g.hubs.cpu()[:, 0].tolist() == [0] and g.t_n_slots == 7 and g.t_hubs.cpu()[:, 0].tolist() == [1]
    assert whole.graph(torch.device(DEV)).n_slots == 0
    a, b, w = (run_layer(small, FIVE, x, cot, cot_k), run_layer(small, FIVE, x, cot, cot_k), run_layer(whole, FIVE, x, cot, cot_k))
    assert equal_runs(a, b)                                   # fixed slot order, no atomics: bit-equal runs
    want, truth = oracles(("hub", H), x, small, FIVE, _HUB, "sigmoid", cot, cot_k)
    compare(a, want, truth, FIVE, "bf16/hub/H%d/chunk32" % H)
    compare(w, want, truth, FIVE, "bf16/hub/H%d/whole" % H)
    as_np = lambda r: {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in r.items()}
    compare(a, as_np(w), truth, FIVE, "bf16/hub/H%d/chunk32-vs-whole" % H)


# ---- K > 4 and the K-slice loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [EIGHT, EIGHT + ["max2"]], ids=["K8", "K9"])           # 9 masks: two launch groups
def test_many_masks(names):
    H = 20
    layer = make_layer(_BOUNDARY, H, names, "new_sigmoid", chunk=512)
    x, cot, cot_k = inputs(_BOUNDARY, H, len(names))
    got = run_layer(layer, names, x, cot, cot_k)
    want, truth = oracles(("many", len(names)), x, layer, names, _BOUNDARY, "new_sigmoid", cot, cot_k)
    compare(got, want, truth, names, "bf16/K%d" % len(names))


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,graph,chunk", [(20, "boundary", 512), (128, "hub", 32), (6, "hub", 32)])
def test_explicit_keep_mask(H, graph, chunk):
    from mma_amd import functional as Fn
    add_all = _BOUNDARY if graph == "boundary" else _HUB
    E = sum(len(a) for a in add_all)
    keep = torch.from_numpy((np.random.default_rng(5).random((len(FIVE), E, H)) >= 0.5).astype(np.uint8))
    layer = make_layer(add_all, H, FIVE, "sigmoid", 0.5, chunk=chunk)
    layer.drop_override = Fn.DropoutSpec(0.5, keep=keep.to(DEV))
    x, cot, cot_k = inputs(add_all, H, len(FIVE))
    got = run_layer(layer, FIVE, x, cot, cot_k)
    want, truth = oracles(("keep", graph, H), x, layer, FIVE, add_all, "sigmoid", cot, cot_k, keeps=keep, p=0.5)
    compare(got, want, truth, FIVE, "bf16/keep/%s/H%d" % (graph, H))


@pytest.mark.parametrize("H", [128, 6])
def test_hash_dropout_is_repeatable_and_seeded(H):
    from mma_amd import functional as Fn
    p = 0.3                                                   # a threshold that is no multiple of 256 (16-bit form)
    layer = make_layer(_HUB, H, FIVE, "sigmoid", p, chunk=32)
    x, cot, cot_k = inputs(_HUB, H, len(FIVE))
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDEF)
    a, b = run_layer(layer, FIVE, x, cot, cot_k), run_layer(layer, FIVE, x, cot, cot_k)
    assert equal_runs(a, b) and all(bool(torch.isfinite(a[k]).all()) for k in ("m", "msum", "gx", "gx_k"))
    layer.drop_override = Fn.DropoutSpec(p, seed=0x1234567890ABCDF0)
    c = run_layer(layer, FIVE, x, cot, cot_k)
    assert not torch.equal(a["msum"], c["msum"]) and not torch.equal(a["gx"], c["gx"]) and not torch.equal(a["m"], c["m"])
    layer.drop_override = Fn.DropoutSpec(0.0)
    assert not torch.equal(a["msum"], run_layer(layer, FIVE, x, cot, cot_k)["msum"])


# ---- the one-launch small-graph form and the unfused node backward ----------------------------------------------------------------
def test_one_launch_and_unfused_node_backward_give_equal_results(monkeypatch):
    from mma_amd import functional as Fn, graph as G
    H, names = 20, ["sum", "mean3", "max", "min"]             # one K-slice: the plan the one-launch form takes
    layer = make_layer(_SMALL_HUB, H, names, "sigmoid", 0.5, chunk=32)
    layer.drop_override = Fn.DropoutSpec(0.5, seed=77)
    x, cot, cot_k = inputs(_SMALL_HUB, H, len(names))
    graph = layer.graph(torch.device(DEV))
    assert graph.n_slots == 2 and graph.t_n_slots == 2 and 0 < graph.n_wave_items < graph.items.shape[0]
    res = {}
    for one in (True, False):
        for fuse in (True, False):
            monkeypatch.setattr(G, "ONE_LAUNCH", one)
            monkeypatch.setattr(Fn, "FUSE_NODE_BWD", fuse)
            assert (graph.sync(0) is not None) == one and (graph.sync(1) is not None) == one
            res[one, fuse] = run_layer(layer, names, x, cot, cot_k)
    for key in res:
        assert equal_runs(res[key], res[True, True]), "ONE_LAUNCH=%s FUSE_NODE_BWD=%s differs" % key
    # and the same plan without dropout against the oracle
    layer.drop_override = Fn.DropoutSpec(0.0)
    monkeypatch.setattr(G, "ONE_LAUNCH", True)
    monkeypatch.setattr(Fn, "FUSE_NODE_BWD", True)
    got = run_layer(layer, names, x, cot, cot_k)
    want, truth = oracles(("small", H), x, layer, names, _SMALL_HUB, "sigmoid", cot, cot_k)
    compare(got, want, truth, names, "bf16/small/one-launch")


# ---- through the layer ------------------------------------------------------------------------------------------------------------
def saved_tables(out):
    """The bf16 tensors an autograd graph keeps for its backward."""
    found, seen, todo = [], set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        found += [t for t in getattr(fn, "saved_tensors", ()) if t is not None and t.dtype == BF16]
        todo += [f for f, _ in fn.next_functions]
    return found


def layer_tail_oracle(layer, names, x, add_all, A64, cot, dtype, table_dtype=BF16, activation="sigmoid"):
    """A (c (msum W)) + b and its gradients with respect to x, the mask weights, W and b."""
    N = len(add_all)
    factor = layer._scaler_factor(N, torch.device(DEV)).detach().cpu().reshape(-1, 1).to(dtype)
    xo = x.to(dtype).requires_grad_(True)
    leaves = [w.detach().cpu().to(dtype).requires_grad_(True) for w in weights(layer, names) + [layer.weight, layer.bias]]
    msum = fused_oracle(xo, leaves[:len(names)], names, add_all, activation, table_dtype=table_dtype).sum(0)
    out = A64.to(dtype) @ (factor * (msum @ leaves[-2])) + leaves[-1]
    grads = torch.autograd.grad((out * cot.to(dtype)).sum(), [xo] + leaves)
    return [out.detach().numpy(), msum.detach().numpy()] + [g.numpy() for g in grads]


def test_layer_forward_and_parameter_gradients():
    H, names = 20, ["sum", "mean3", "max", "softmax"]
    A64, adj = normalized_adj(_SMALL)
    layer = make_layer(_SMALL, H, names, "sigmoid", 0.0)
    x, _, _ = inputs(_SMALL, H, len(names))
    cot = torch.from_numpy(np.random.default_rng(8).standard_normal((len(_SMALL), C_OUT)).astype(np.float32))
    xg = x.to(DEV).requires_grad_(True)
    params = weights(layer, names) + [layer.weight, layer.bias]
    out = layer(xg, adj)
    tables = saved_tables(out)
    assert len(tables) == 1 and tables[0].shape == (len(_SMALL), 2 * len(names) * H)          # the [P | Q] buffer, in bf16, and only it
    grads = torch.autograd.grad((out * cot.to(DEV)).sum(), [xg] + params)
    # the grids make the forward GEMM exact: the table the kernels read is the oracle's, bit for bit (module docstring)
    Ws = [w.detach().cpu() for w in weights(layer, names)]
    pq = torch.cat([x @ w[:H] for w in Ws] + [x @ w[H:] for w in Ws], 1)
    assert torch.equal(tables[0].cpu().view(torch.int16), pq.to(BF16).view(torch.int16))
    assert torch.equal(pq.double(), torch.cat([x.double() @ w[:H].double() for w in Ws] + [x.double() @ w[H:].double() for w in Ws], 1))
    want = layer_tail_oracle(layer, names, x, _SMALL, A64, cot, torch.float32)
    truth = layer_tail_oracle(layer, names, x, _SMALL, A64, cot, torch.float64)
    got = [out.detach()] + list(grads)
    tags = ["out", "gx"] + ["gmask[%s]" % n for n in names] + ["gweight", "gbias"]
    for g, w, t, tag in zip(got, [want[0]] + want[2:], [truth[0]] + truth[2:], tags):
        if tag == "gbias":
            g, w, t = g.reshape(1, -1), w.reshape(1, -1), t.reshape(1, -1)
        print("bf16/layer/%s: max |got - fp64| %.3g" % (tag, np.abs(g.detach().cpu().numpy() - t).max()))
        check_close(g, w, None, None, what="bf16/layer/" + tag, signed_sum=True, truth=t)


def test_layer_trains_a_step():
    H, names = 20, ["sum", "mean3", "max", "softmax"]
    _, adj = normalized_adj(_SMALL)
    layer = make_layer(_SMALL, H, names, "new_sigmoid", 0.5)
    x, _, _ = inputs(_SMALL, H, len(names))
    params = weights(layer, names) + [layer.weight, layer.bias]
    opt = torch.optim.SGD(params, lr=0.1)
    before = [p.detach().clone() for p in params]
    out = layer(x.to(DEV), adj)
    assert out.shape == (len(_SMALL), C_OUT)
    out.square().mean().backward()
    opt.step()
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) and not torch.equal(p.detach(), b)
    assert bool(torch.isfinite(layer(x.to(DEV), adj)).all())


def test_graph_capture_replays_with_fresh_dropout_bits():
    H, names = 20, ["sum", "mean3", "max"]
    _, adj = normalized_adj(_SMALL)
    layer = make_layer(_SMALL, H, names, "sigmoid", 0.5)
    layer.graph_capturable = True
    x = inputs(_SMALL, H, len(names))[0].to(DEV).requires_grad_(True)
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
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_static = step()
    outs, seeds = [], []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        outs.append((out_static.clone(), x.grad.clone()))
        seeds.append(layer._seed_buf.cpu().tolist())
    assert seeds[0] != seeds[1]
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    assert all(bool(torch.isfinite(t).all()) for o in outs for t in o)


# ---- bf16 is really used ------------------------------------------------------------------------------------------------------------
def test_the_saved_table_is_bf16_and_the_fp32_layer_saves_none():
    H, names = 20, ["sum", "max"]
    x = inputs(_SMALL, H, len(names))[0].to(DEV).requires_grad_(True)
    half = make_layer(_SMALL, H, names)
    full = make_layer(_SMALL, H, names, logit_dtype=torch.float32)
    assert half.logit_dtype == BF16 and full.logit_dtype == torch.float32
    for reduce_k, n_tables in ((True, 1), (False, 2)):                 # [P | Q] in one buffer / P and Q
        t = saved_tables(half._aggregate_all(names, x, reduce_k=reduce_k))
        assert len(t) == n_tables and all(u.dtype == BF16 for u in t)
        assert saved_tables(full._aggregate_all(names, x, reduce_k=reduce_k)) == []
    assert saved_tables(half.learnable_max(x, None))[0].shape == (len(_SMALL), H)


def test_large_logits_show_the_rounding_and_match_the_bf16_oracle():
    """Mask weights scaled by 16: |z| reaches 8 and beyond, a bf16 step there is 2^-5.  The bf16 layer then differs from the fp32 layer by
    far more than the fp32 bar allows - and still meets that bar against the oracle that rounds the same tables."""
    H, names = 20, ["sum", "mean3"]
    half = make_layer(_SMALL, H, names, "new_sigmoid", scale=16.0)
    full = make_layer(_SMALL, H, names, "new_sigmoid", scale=16.0, logit_dtype=torch.float32)
    x, cot, cot_k = inputs(_SMALL, H, len(names))
    Ws = [w.detach().cpu() for w in weights(half, names)]
    z_max = max(float((x @ w[:H]).abs().max() + (x @ w[H:]).abs().max()) for w in Ws)
    assert z_max >= 8.0, z_max
    got_h, got_f = run_layer(half, names, x, cot, cot_k), run_layer(full, names, x, cot, cot_k)
    want, truth = oracles(("large", "bf16"), x, half, names, _SMALL, "new_sigmoid", cot, cot_k)
    compare(got_h, want, truth, names, "bf16/large-logits")
    w32, t32 = [oracle_with_grads(x, Ws, names, _SMALL, "new_sigmoid", cot, cot_k, dtype=dt, table_dtype=torch.float32)
                for dt in (torch.float32, torch.float64)]
    compare(got_f, w32, t32, names, "fp32/large-logits", parts=("msum",))
    with pytest.raises(AssertionError, match="outside"):
        compare(got_h, w32, t32, names, "bf16-vs-fp32-oracle/large-logits", parts=("msum",))
    diff = (got_h["msum"] - got_f["msum"]).abs().max().item()
    print("large logits: max |z| %.3g, max |msum(bf16) - msum(fp32)| %.3g" % (z_max, diff))
    assert diff > 1e-3


# ---- default unchanged ------------------------------------------------------------------------------------------------------------
def test_float32_keyword_equals_no_keyword_bit_for_bit():
    import mma_amd
    H, names = 20, FIVE
    x, cot, cot_k = inputs(_HUB, H, len(names))
    explicit = make_layer(_HUB, H, names, "sigmoid", chunk=32, logit_dtype=torch.float32)
    torch.manual_seed(0)
    P = lambda *s: torch.nn.Parameter(torch.empty(*s, device=DEV))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    plain = mma_amd.MMA(_HUB, "sigmoid", 2, H, C_OUT, P(H, C_OUT), P(C_OUT), *masks, 0.0, list(names), DEV, chunk=32)       # no keyword
    with torch.no_grad():
        for n in ALL_MASK_NAMES:
            getattr(plain, "mask_" + n).copy_(getattr(explicit, "mask_" + n))
    assert plain.logit_dtype == torch.float32
    assert equal_runs(run_layer(explicit, names, x, cot, cot_k), run_layer(plain, names, x, cot, cot_k))
