"""GPU tests of the bf16-output form of the three-product column-group GEMMs (ABI 39: mma_gemm_f16x2_k_h / _k256_h / _k256p_h;
dense.gemm_f16x2(out_dtype=), a bf16 `out` of dense.mm_into, and MMA(..., logit_dtype=torch.bfloat16), whose forward GEMM now leaves
[P|Q] in bf16 from its own epilogue).

Every comparison is on bits (view(torch.int16), torch.equal): no tolerance is involved.  The reference never involves the new kernels:
it is the UNCHANGED fp32 kernel's output converted by torch (.to(torch.bfloat16), round to nearest even) - the bf16 kernels run the
fp32 kernels' code up to the value they store, so the two must agree on every non-NaN element, and be NaN at the same places (NaN bits
are not compared).  Shapes are the smallest at which the kernels take another path: less than one wave's 32 rows, one full 256-row
unit plus a ragged one, the first size the layer's dispatch admits (4099), every (G2, K) instantiation; the fp32 references are
computed once per shape and shared."""
import functools

import numpy as np
import pytest
import torch

from golden.inputs import ALL_MASK_NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
SENTINEL = 0x7B7B                      # bf16 bit pattern of the guard cells (a large finite number no product below produces)
C_OUT = 4


def bits(t):
    return t.contiguous().view(torch.int16)


def assert_same_bf16(got, want, what=""):
    """Bit equality of two bf16 tensors outside their NaNs, which must sit at the same places."""
    assert got.dtype == BF16 and want.dtype == BF16 and got.shape == want.shape, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaNs at different places (%d vs %d)" % (what, int(gn.sum()), int(wn.sum()))
    g, w = bits(got).masked_fill(gn, 0), bits(want).masked_fill(wn, 0)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %r: got %r want %r"
                             % (what, len(bad), g.numel(), i, got[i].item(), want[i].item()))


def guarded(M, N):
    """(buffer, out): out (M, N) is a column block of a wider bf16 buffer - row pitch N + 8 (3 guard columns left, 5 right: the block
    starts on a 2-byte boundary only, the form's stated alignment), 8 guard rows above and 32 below (a wave re-reads up to 31 rows past
    M, whose stores only the descriptor's range keeps out), every guard cell = SENTINEL."""
    buf = torch.full((M + 40, N + 8), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
    return buf, buf[8:8 + M, 3:3 + N]


def assert_guards_intact(buf, M, N, what=""):
    b = bits(buf).clone()
    b[8:8 + M, 3:3 + N] = SENTINEL
    assert bool((b == SENTINEL).all()), "%s: %d guard cells overwritten" % (what, int((b != SENTINEL).sum()))


# ---- direct calls to dense.gemm_f16x2 ---------------------------------------------------------------------------------------------
KS, NS, MS = (64, 96, 128), (128, 256, 384), (31, 293, 4099)


@functools.lru_cache(maxsize=None)
def case(K, N, M):
    """(a, w, fp32 result of the unchanged kernel, its row maxima).  `a` is a row-strided view (a column block of a wider buffer) with an
    all-zero row, a row of 1e36, a row of 1e-30, a row whose products overflow to inf, and a NaN row."""
    from mma_amd import dense
    rng = np.random.default_rng(1000 * K + N + M)
    wide = torch.from_numpy(rng.standard_normal((M, K + 8)).astype(np.float32))
    wide[0] = 0.0
    wide[1] = 1e36
    wide[2] = 1e-30
    wide[3] *= 3e38 / wide[3].abs().max()
    wide[4] = float("nan")
    a = wide.to(DEV)[:, :K]
    assert a.stride(0) == K + 8
    w = torch.from_numpy((rng.standard_normal((K, N)) * 4.0).astype(np.float32)).to(DEV)
    rm = torch.empty(M, device=DEV)
    ref = dense.gemm_f16x2(a, w, row_max_out=rm)
    assert ref.dtype == torch.float32
    assert bool(torch.isinf(ref[3]).any()) and bool(torch.isnan(ref[4]).any()) and bool((ref[0] == 0).all())      # the inputs do what they are for
    return a, w, ref, rm


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_every_instantiation_equals_the_converted_fp32_result(K, N, M):
    from mma_amd import dense
    a, w, ref, _ = case(K, N, M)
    got = dense.gemm_f16x2(a, w, out_dtype=BF16)
    assert got.dtype == BF16 and got.shape == (M, N)
    assert_same_bf16(got, ref.to(BF16), "K=%d N=%d M=%d" % (K, N, M))
    again = dense.gemm_f16x2(a, w, out=torch.empty((M, N), device=DEV, dtype=BF16))        # a given `out` decides by its own dtype
    assert_same_bf16(again, got, "given out")


@pytest.mark.parametrize("g2", [None, "1"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N", [(64, 384), (96, 256), (128, 256), (128, 128)])
def test_nothing_outside_the_result_is_written(K, N, M, g2, monkeypatch):
    from mma_amd import dense
    if g2 is not None:
        monkeypatch.setenv("MMA_F16X2_G2", g2)               # one resident column group per workgroup (read per call)
    a, w, ref, _ = case(K, N, M)
    buf, out = guarded(M, N)
    assert out.stride(0) == N + 8 and out.data_ptr() % 4 == 2
    res = dense.gemm_f16x2(a, w, out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_same_bf16(out, ref.to(BF16), "K=%d N=%d M=%d G2=%s" % (K, N, M, g2))
    assert_guards_intact(buf, M, N)


@pytest.mark.parametrize("K,N,M", [(64, 384, 293), (96, 128, 31), (128, 256, 4099)])
def test_row_maxima_equal_those_of_the_fp32_call(K, N, M):
    from mma_amd import dense
    a, w, _, rm32 = case(K, N, M)
    rm = torch.full((M,), -1.0, device=DEV)
    dense.gemm_f16x2(a, w, row_max_out=rm, out_dtype=BF16)
    assert torch.equal(torch.isnan(rm), torch.isnan(rm32))
    assert torch.equal(torch.nan_to_num(rm, nan=-2.0), torch.nan_to_num(rm32, nan=-2.0))
    assert torch.equal(rm[5:], a[5:].abs().amax(1))


def test_ties_round_to_even():
    """Integer operands (|a|, |w| <= 8): every product and sum is exact in fp32 (and in the fp16 pieces), so the value before rounding
    is the integer a @ w, and an odd integer above 256 lies exactly half-way between two bf16 numbers."""
    from mma_amd import dense
    K, N, M = 64, 128, 293
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.integers(-8, 9, (M, K)).astype(np.float32)).to(DEV)
    w = torch.from_numpy(rng.integers(-8, 9, (K, N)).astype(np.float32)).to(DEV)
    exact = (a.double() @ w.double())
    assert bool(((exact.abs() > 256) & (exact.abs() < 512) & (exact.long() % 2 == 1)).any()), "no tie among the outputs"
    assert torch.equal(dense.gemm_f16x2(a, w).double(), exact)                       # the fp32 kernel is exact here
    assert_same_bf16(dense.gemm_f16x2(a, w, out_dtype=BF16), exact.float().to(BF16), "ties")


# ---- through dense.mm_into --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k256_operands():
    M = 65573                                   # the K = 256 forms admit M >= 65536; 65573 = 256 full units + 37 rows
    g = torch.Generator().manual_seed(17)
    a = torch.randn(M, 256, generator=g).to(DEV)
    a[5] = 0.0
    a[6] *= 1e30
    w = {N: (torch.randn(256, N, generator=g) * 0.25).to(DEV) for N in (128, 384)}
    return a, w


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("N", [128, 384])
def test_k256_forms_equal_the_converted_fp32_result(N, packed, monkeypatch):
    from mma_amd import dense
    monkeypatch.setattr(dense, "PACK_K256", packed)
    a, ws = k256_operands()
    M, w = a.shape[0], ws[N]
    if N == 384:                                # (N = 128 is not a column-group shape at K = 256: it takes the fallback, same bits)
        assert dense.nn_form(M, 256, N) == ("f16x2_k256p" if packed else "f16x2_k256")
    ref = dense.mm_into(a, w, torch.empty((M, N), device=DEV))
    buf, out = guarded(M, N)
    box = []
    dense.mm_into(a, w, out, row_max_box=box)
    torch.cuda.synchronize()
    assert_same_bf16(out, ref.to(BF16), "K=256 N=%d packed=%s" % (N, packed))
    assert_guards_intact(buf, M, N)
    if N == 384:
        assert len(box) == 1 and torch.equal(box[0], a.abs().amax(1))


@pytest.mark.parametrize("M,K,N,form", [(1000, 128, 256, "lib"), (5000, 256, 64, "bf16x3")])
def test_forms_without_a_bf16_epilogue_convert_an_fp32_product_once(M, K, N, form, monkeypatch):
    from mma_amd import dense
    from mma_amd import functional as Fn
    assert dense.nn_form(M, K, N) == form
    g = torch.Generator().manual_seed(M)
    a, w = torch.randn(M, K, generator=g).to(DEV), torch.randn(K, N, generator=g).to(DEV)
    ref = dense.mm_into(a, w, torch.empty((M, N), device=DEV))
    calls, real = [], Fn.rows_to_bf16
    monkeypatch.setattr(Fn, "rows_to_bf16", lambda *args, **kw: (calls.append(1), real(*args, **kw))[1])
    buf, out = guarded(M, N)
    dense.mm_into(a, w, out)
    torch.cuda.synchronize()
    assert len(calls) == 1
    assert_same_bf16(out, ref.to(BF16), form)
    assert_guards_intact(buf, M, N)


# ---- the layer: MMA(..., logit_dtype=torch.bfloat16) ------------------------------------------------------------------------------------
def random_graph(N, seed=3):
    """Mean degree 4, one hub of degree 600 (half the nodes where the graph has fewer than 1200)."""
    rng = np.random.default_rng(seed)
    add_all = [sorted(set(rng.integers(0, N, rng.poisson(4)).tolist())) for _ in range(N)]
    add_all[7] = sorted(rng.choice(N, size=min(600, N // 2), replace=False).tolist())
    return add_all


def adjacency(add_all):
    """Row-normalised A + I as a sparse tensor."""
    N = len(add_all)
    nb = [sorted(set(a) | {i}) for i, a in enumerate(add_all)]
    rows = np.concatenate([np.full(len(n), i, dtype=np.int64) for i, n in enumerate(nb)])
    cols = np.concatenate([np.asarray(n, dtype=np.int64) for n in nb])
    vals = np.concatenate([np.full(len(n), 1.0 / len(n), np.float32) for n in nb])
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(vals), (N, N)).coalesce().to(DEV)


@functools.lru_cache(maxsize=None)
def layer_setup(N, H, K, p=0.5):
    import mma_amd
    add_all = random_graph(N)
    names = ["sum", "mean", "max", "min"][:K]
    torch.manual_seed(N + H)
    P = lambda *s: torch.nn.Parameter(torch.empty(*s, device=DEV))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    layer = mma_amd.MMA(add_all, "sigmoid", 2, H, C_OUT, P(H, C_OUT), P(C_OUT), *masks, p, names, DEV, logit_dtype=BF16)
    x = torch.randn(N, H).to(DEV).requires_grad_(True)
    cot = torch.randn(N, C_OUT).to(DEV)
    return layer, names, x, cot, adjacency(add_all)


def saved_bf16(out):
    found, seen, todo = [], set(), [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        found += [t for t in getattr(fn, "saved_tensors", ()) if t is not None and t.dtype == BF16]
        todo += [f for f, _ in fn.next_functions]
    return found


def layer_step(layer, names, x, cot, adj):
    from mma_amd import functional as Fn
    params = [layer.weight, layer.bias] + [getattr(layer, "mask_" + n) for n in names]
    layer.drop_override = Fn.DropoutSpec(layer.dropout, seed=0x5EED5EED) if layer.dropout > 0 else None
    out = layer(x, adj)
    tables = saved_bf16(out)
    grads = torch.autograd.grad((out * cot).sum(), [x] + params)
    torch.cuda.synchronize()
    return [out.detach()] + list(grads), tables


def count_conversions(monkeypatch):
    from mma_amd import functional as Fn
    calls, real = [], Fn.rows_to_bf16
    monkeypatch.setattr(Fn, "rows_to_bf16", lambda *args, **kw: (calls.append(1), real(*args, **kw))[1])
    return calls


@pytest.mark.parametrize("H,K,form", [(64, 3, "lib"), (128, 4, "f16x2_k")])          # 2 K H = 384, 1024
def test_layer_with_bf16_epilogue_equals_the_conversion_pass(H, K, form, monkeypatch):
    """dense.BF16_EPILOGUE on against off (MMA_BF16_EPILOGUE=0: the fp32 product + mma_rows_to_bf16): the output, dL/dx and the
    gradients of the weight, the bias and every mask are the same bits, and the saved [P|Q] is bf16 either way.  At H = 128 the forward
    product runs on the whole-row three-product kernel (two resident column groups): on, no conversion runs at all.  At H = 64 nn_form
    sends the layer's product to the library (its admission wants K % 128 == 0 outside the named calls; the narrow kernels with three
    resident groups are reached through gemm_bf16x3 / gemm_f16x2, see the direct tests above), so this shape converts once on both sides
    - the selection is not this feature's to change."""
    from mma_amd import dense
    N = 4099
    layer, names, x, cot, adj = layer_setup(N, H, K)
    assert dense.nn_form(N, H, 2 * K * H) == form
    calls = count_conversions(monkeypatch)
    monkeypatch.setattr(dense, "BF16_EPILOGUE", True)
    on, tables = layer_step(layer, names, x, cot, adj)
    assert len(calls) == (0 if form in dense._BF16_OUT_FORMS else 1)
    assert [tuple(t.shape) for t in tables] == [(N, 2 * K * H)]
    del calls[:]
    monkeypatch.setattr(dense, "BF16_EPILOGUE", False)
    off, tables_off = layer_step(layer, names, x, cot, adj)
    assert len(calls) == 1 and [tuple(t.shape) for t in tables_off] == [(N, 2 * K * H)]
    assert_same_bf16(tables[0], tables_off[0], "saved [P|Q]")
    for what, g, w in zip(["out", "dL/dx", "weight", "bias"] + names, on, off):
        assert bool(torch.isfinite(g).all()) and torch.equal(g, w), what


def test_a_graph_too_small_for_the_epilogue_forms_takes_the_conversion(monkeypatch):
    from mma_amd import dense
    N, H, K = 300, 64, 3
    layer, names, x, cot, adj = layer_setup(N, H, K)
    assert dense.nn_form(N, H, 2 * K * H) == "lib"
    calls = count_conversions(monkeypatch)
    monkeypatch.setattr(dense, "BF16_EPILOGUE", True)
    on, tables = layer_step(layer, names, x, cot, adj)
    assert len(calls) == 1 and [tuple(t.shape) for t in tables] == [(N, 2 * K * H)]          # the fallback is reached
    monkeypatch.setattr(dense, "BF16_EPILOGUE", False)
    off, _ = layer_step(layer, names, x, cot, adj)
    assert len(calls) == 2
    for g, w in zip(on, off):
        assert torch.equal(g, w)


@pytest.mark.parametrize("H,K", [(64, 3), (128, 4)])          # (the library product + the conversion, the bf16 epilogue: see above)
def test_graph_capture_replays_the_eager_result(H, K, monkeypatch):
    from mma_amd import dense
    monkeypatch.setattr(dense, "BF16_EPILOGUE", True)
    N = 4099
    layer, names, x, cot, adj = layer_setup(N, H, K, 0.0)
    params = [layer.weight, layer.bias] + [getattr(layer, "mask_" + n) for n in names]

    def step():
        x.grad = None
        for prm in params:
            prm.grad = None
        out = layer(x, adj)
        out.backward(cot)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                       # warm-up: plans and caches
            eager = step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    want = [eager.detach().clone(), x.grad.clone()] + [prm.grad.clone() for prm in params]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_static = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got = [out_static, x.grad] + [prm.grad for prm in params]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
