"""The segmented kernels at the thresholds where their structure switches, with row layouts built on purpose rather than drawn at random:

- the block segment sum (spmm_rows.hip, segsum_block_kernel): kSegRows = 16 rows per workgroup, rows above kSegLong = 64 edges go to a
  column-parallel tail, blocks of more than kSegCap = 512 edges read their edge ids from memory, and the kernel is taken for
  32 <= C and 16 * C * 4 <= 64 KiB only;
- the GR block kernels (gr_fused.hip, gr_fwd_block_kernel / gr_bwd_block_kernel): nb nodes per workgroup (MMA_GR_NB), segments above
  kGroupMaxDeg = 64 edges go to the wave-per-node pass (the long-node list, or the generic kernel without one), blocks of more than
  kBlkCap = 256 edges are not staged in LDS, and the backward block kernel takes K * S <= kBlkMaxKS = 8 only;
- the tall Linear past 4096 outputs, where the narrow-K three-product kernel no longer takes the product."""
import numpy as np
import pytest
import torch

from golden_util import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEG_ROWS, SEG_LONG = 16, 64                        # spmm_rows.hip: kSegRows, kSegLong


def degrees(blocks, width):
    """Per-row degrees from a list of blocks: each block is a list of at most `width` degrees, placed at the start of its own
    `width`-row slot (the rest of the slot is empty), so that every pattern lands in the workgroup it names."""
    deg = np.zeros(len(blocks) * width, np.int64)
    for i, blk in enumerate(blocks):
        assert len(blk) <= width
        deg[i * width:i * width + len(blk)] = blk
    return deg


def csr(deg, n_src, rng):
    """rowptr (int32) and the source row of every edge (int32, drawn from n_src rows)."""
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    return rowptr, rng.integers(0, n_src, int(rowptr[-1])).astype(np.int32)


# ---- A. the segment sum ----------------------------------------------------------------------------------------------------------------

def sequential_sum(rowptr, idx, src, C, dtype=np.float32):
    """out[r] = (((0 + B[idx[b]]) + B[idx[b+1]]) + ...) in `dtype`: sequential per row in edge order, vectorised over rows by edge slot."""
    deg = np.diff(rowptr)
    acc = np.zeros((len(deg), C), dtype)
    for t in range(int(deg.max()) if len(deg) else 0):
        r = np.nonzero(deg > t)[0]
        acc[r] = acc[r] + src[idx[rowptr[r] + t], :C].astype(dtype)
    return acc


def segsum(rowptr, idx, src, C, row_max=None):
    """mma_csr_spmm (or mma_csr_spmm_rm with a zeroed row_max) into a NaN-filled output; ldb = the source table's row pitch."""
    from mma_amd._lib import call, ptr, stream_ptr
    n_rows = len(rowptr) - 1
    B = torch.from_numpy(src).to(DEV)
    out = torch.full((n_rows, C), float("nan"), device=DEV)
    args = (ptr(torch.from_numpy(rowptr).to(DEV)), ptr(torch.from_numpy(idx).to(DEV)), None, ptr(B), src.shape[1], int(rowptr[-1]), 1, None,
            ptr(out), C, n_rows, C)
    if row_max is None:
        call("mma_csr_spmm", *args, stream_ptr())
    else:
        call("mma_csr_spmm_rm", *args, ptr(row_max), stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def in_edge_order(C):
    """Whether mma_csr_spmm adds a row's members sequentially in edge order at width C: the block kernel always; the wave-per-row kernel
    when one row's columns take the whole wavefront (C / 4 > 32 float4 lanes).  Narrower, the wave kernel gathers 64 / LPR edges per step
    in LPR-lane groups and adds the groups' partial sums in a butterfly - a different order."""
    block = C % 4 == 0 and 32 <= C and SEG_ROWS * C * 4 <= 64 * 1024
    return block or C // 4 > 32


def assert_segsum(got, rowptr, idx, src, C, what, ordered=None):
    """Bit for bit the sequential fp32 sum where the kernel adds in edge order (`ordered`, default: in_edge_order(C)), else within the
    summation bound of any order."""
    want = sequential_sum(rowptr, idx, src, C)
    if in_edge_order(C) if ordered is None else ordered:
        bad = np.argwhere(~(got == want))
        assert bad.size == 0, "%s: %d elements differ from the sequential fp32 sum, first rows %s" % (what, len(bad), np.unique(bad[:, 0])[:8])
        return
    # another order of the same additions: within the bound of any fp32 summation order, (deg - 1) u sum |x| (u = 2^-24)
    exact = sequential_sum(rowptr, idx, src, C, np.float64)
    mag = sequential_sum(rowptr, idx, np.abs(src), C, np.float64)
    deg = np.diff(rowptr)[:, None].astype(np.float64)
    assert not np.isnan(got).any(), what + ": NaN left in the output"
    assert bool((np.abs(got - exact) <= np.maximum(deg - 1, 0) * 2.0 ** -24 * mag * 1.01).all()), what + ": beyond the fp32 summation bound"


def race_blocks(long_at):
    """The layout of the long-row race: eight empty rows, seven rows of exactly kSegLong edges (the wavefront that owns them spends ~60
    dependent gathers in its item loop) and one row of kSegLong + 1 edges whose column-parallel tail other lanes finish first - at block
    position 15 (long_at = 15) or, mirrored, at position 0.  513 edges: just past kSegCap, so the edge ids come from memory."""
    blk = [0] * 8 + [SEG_LONG] * 7 + [SEG_LONG + 1]
    return blk if long_at == 15 else blk[::-1]


@pytest.mark.parametrize("C,long_at,n_blocks", [(32, 15, 2048), (380, 15, 1024), (380, 0, 1024)])
def test_segsum_long_row_tail_is_not_overwritten(C, long_at, n_blocks):
    """The item loop of segsum_block_kernel must leave rows above kSegLong to the tail: it once stored its zero accumulator for them too,
    with no barrier before the tail wrote the real sum into the same LDS cells from other lanes.  C = 32: items = 128, so wavefronts 2-3
    idle and row 15's items sit in wavefront 1 behind the seven 64-edge rows, while lanes 0-7 of wavefront 0 run the tail.  Thousands of
    workgroups in one launch; every row bit for bit the sequential sum."""
    rng = np.random.default_rng(C + long_at)
    deg = degrees([race_blocks(long_at)] * n_blocks, SEG_ROWS)
    rowptr, idx = csr(deg, 4096, rng)
    src = rng.standard_normal((4096, C)).astype(np.float32)
    got = segsum(rowptr, idx, src, C)
    assert_segsum(got, rowptr, idx, src, C, "race layout C=%d long row at %d" % (C, long_at))


SEG_CATALOGUE = [                                    # one block of kSegRows rows each; the comment names the threshold it targets
    [0, 1, 2, 3, 4, 5, 1, 2, 0, 3, 1, 1, 2, 0, 4, 1],                   # short rows only (the fixed four-slot batch, clamped)
    [63, 64, 65, 66] + [1] * 12,                                         # degrees around kSegLong: 63 / 64 item loop, 65 / 66 tail
    [SEG_LONG] * 7 + [SEG_LONG - 1],                                     # 511 edges: staged, no long row
    [SEG_LONG] * 8,                                                      # 512 = kSegCap: staged, no long row
    [SEG_LONG] * 8 + [1],                                                # 513: ids from memory, no long row
    [65] + [SEG_LONG] * 6 + [62],                                        # 511 with a long row at position 0
    [65] + [SEG_LONG] * 6 + [63],                                        # 512 with a long row
    [0] * 8 + [SEG_LONG] * 6 + [64, 65],                                 # 513 with a long row at position 15
    [],                                                                  # whole blocks of empty rows in the middle ...
    [],
    [100] + [1] * 7 + [64] + [0] * 6 + [70],                             # two long rows in one block, one at each end, a 64-edge row
    [200, 200, 3],                                                       # two long rows side by side, 403 edges (staged)
    [0] * 15 + [300],                                                    # one long row behind 15 empty ones, 300 edges (staged)
    [600],                                                               # one row longer than kSegCap: ids from memory, tail only
    list(range(16)),
    [],                                                                  # ... and at the end (before the partial tail block)
]


@pytest.mark.parametrize("C,pad,tail", [(32, 0, 15), (32, 4, 1), (380, 0, 1), (380, 4, 15), (1024, 0, 15), (28, 0, 1), (1028, 4, 15)])
def test_segsum_at_the_thresholds(C, pad, tail, monkeypatch):
    """Every block pattern of SEG_CATALOGUE (each in its own workgroup) in one launch, repeated; a last, partial block of 1 or 15 rows
    (n_rows % 16); strided source rows (pad: ldb = C + 4).  C = 32 / 1024 are the narrowest and widest widths of the block kernel, 28 and
    1028 fall just outside its gate (the wave-per-row kernel).  Checked: the sequential fp32 sum, the wave-per-row kernel on the same inputs
    (MMA_SEGSUM_BLOCK=0, read per call: the same bits where it adds in edge order too), and mma_csr_spmm_rm - the same output, and row
    maxima equal to max |row| exactly."""
    rng = np.random.default_rng(C * 10 + pad + tail)
    deg1 = degrees(SEG_CATALOGUE, SEG_ROWS)
    reps = max(1, 20_000_000 // (int(deg1.sum()) * C))           # keeps the host reference at ~20 M gathered floats
    deg = np.concatenate([np.tile(deg1, reps), rng.integers(0, 6, tail)])
    deg[-1] = 70 if tail == 15 else deg[-1]                      # a long row in the partial block
    rowptr, idx = csr(deg, 2048, rng)
    src = rng.standard_normal((2048, C + pad)).astype(np.float32)
    what = "segsum C=%d ldb=%d n_rows=%d" % (C, C + pad, len(deg))
    got = segsum(rowptr, idx, src, C)
    assert_segsum(got, rowptr, idx, src, C, what)
    rm = torch.zeros(len(deg), device=DEV)
    got_rm = segsum(rowptr, idx, src, C, row_max=rm)
    assert np.array_equal(got_rm, got), what + ": mma_csr_spmm_rm output differs from mma_csr_spmm"
    assert np.array_equal(rm.cpu().numpy(), np.abs(got).max(1)), what + ": row maxima are not max |row|"
    monkeypatch.setenv("MMA_SEGSUM_BLOCK", "0")
    got_wave = segsum(rowptr, idx, src, C)
    assert_segsum(got_wave, rowptr, idx, src, C, what + " (wave-per-row kernel)", ordered=C // 4 > 32)


@pytest.mark.parametrize("blk", [[3], [70], [0, 65, 1, 64, 0], [64] * 15, [0] * 14 + [65]])
def test_segsum_fewer_rows_than_one_block(blk):
    """n_rows < kSegRows: the only workgroup is partial (row pointers past n_rows are never staged)."""
    rng = np.random.default_rng(len(blk) + sum(blk))
    deg = np.array(blk, np.int64)
    rowptr, idx = csr(deg, 64, rng)
    src = rng.standard_normal((64, 380)).astype(np.float32)
    got = segsum(rowptr, idx, src, 380)
    assert_segsum(got, rowptr, idx, src, 380, "segsum n_rows=%d" % len(blk))


# ---- B. the GR block kernels -----------------------------------------------------------------------------------------------------------

# one block of up to 16 targets each (the widest nb): every pattern starts at a multiple of 16, so at nb = 8 / 4 it is the leading block
# of its slot and at nb = 2 it is cut in pairs.  Degrees from {0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 200}.
GR_CATALOGUE = [
    [0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 0, 2, 1, 3, 4],                   # molecule-like short segments (three-slot batch + tail)
    [64, 64, 64, 63],                                                    # 255 edges: staged (kBlkCap - 1)
    [64, 64, 64, 64],                                                    # 256 = kBlkCap: staged
    [64, 64, 64, 65],                                                    # 257 with a long node: ids from memory
    [64, 64, 64, 64, 1],                                                 # 257, no long node (nb = 4: 256 + a block of one edge)
    [200, 66, 64, 3],                                                    # two long nodes next to a 64-edge node (nb = 2: both in one block)
    [63, 64, 65, 66, 5, 4, 3, 2, 1, 0, 0, 1],                            # degrees around kGroupMaxDeg
    [], [],                                                              # 32 empty targets in the middle: whole empty blocks at every nb
    [5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 200],                  # a long node at the far end of a block of empties
    [1, 2, 3, 4, 5, 4, 3, 2, 1, 2, 3, 4, 5, 4, 3, 2],
    [2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2],
    [3] * 16, [2] * 16, [4] * 16, [1] * 16, [5] * 16, [2] * 16, [3] * 16, [4] * 16,     # (keeps E <= 16 N: the block kernels' gate)
    [], [], [],                                                          # 48 empty targets at the end
]


def gr_targets():
    deg = degrees(GR_CATALOGUE, 16)
    assert deg.sum() <= 16 * len(deg)
    return deg


def nb_runs(monkeypatch, run):
    """run() at every MMA_GR_NB (read per call), once with the long-node list and once without it (long_nodes = None: the generic
    wave-per-node kernel behind the block kernel); the two must agree bit for bit, and so must every nb (a node's items do not depend on
    the block it shares).  Returns the results of the first run."""
    first = None
    for nb in (2, 4, 8, 16):
        monkeypatch.setenv("MMA_GR_NB", str(nb))
        for with_list in (True, False):
            res = [t.detach().cpu() for t in run(with_list)]
            if first is None:
                first = res
            else:
                for a, b in zip(res, first):
                    assert torch.equal(a, b), "nb=%d long-node list %s: other bits than nb=2 with the list" % (nb, "on" if with_list else "off")
    return first


@pytest.mark.parametrize("aggs,scalers", [(["min", "max"], ["identity", "amplification", "attenuation", "linear"]),      # K*S = 8: block backward
                                          (["sum", "mean", "max"], ["identity", "amplification", "linear"])])                 # K*S = 9: generic backward
def test_gr_block_aggregate_at_the_thresholds(aggs, scalers, monkeypatch):
    """MMAConv.aggregate (given messages) on GR_CATALOGUE against the oracle: output, dL/dinputs, and the 0/1 gradient of the max
    block bit for bit (ties -> the lowest edge position, also in the wave-per-node pass of the 200-edge nodes)."""
    from mma_amd import functional as Fn
    from oracle import gr_oracle as G
    from test_gr_gpu import make_conv
    T, F = 2, 8
    rng = np.random.default_rng(len(aggs) * 10 + len(scalers))
    deg = gr_targets()
    N = len(deg)
    index = np.repeat(np.arange(N), deg)[rng.permutation(int(deg.sum()))]        # unsorted, as PyG hands it over
    E = len(index)
    vals = rng.integers(-4, 5, (E, T, F)).astype(np.float32) * 0.25                 # many exact ties
    conv = make_conv(aggs, scalers, towers=T, F=F)
    cot = torch.from_numpy(rng.standard_normal((N, T, len(aggs) * len(scalers) * F)).astype(np.float32))
    xi = torch.from_numpy(vals).requires_grad_(True)
    want = G.aggregate(xi, torch.from_numpy(index), N, aggs, scalers, conv.avg_deg)
    gw, = torch.autograd.grad((want * cot).sum(), [xi], retain_graph=True)
    k = aggs.index("max")
    w1, = torch.autograd.grad(want[:, :, k * F:(k + 1) * F].sum(), [xi])
    idx_d = torch.from_numpy(index).to(DEV)
    graph = Fn.GRGraph(torch.stack([idx_d, idx_d]), N)
    long_list = graph.by_target.long_nodes

    def run(with_list):
        graph.by_target.long_nodes = long_list if with_list else None
        xg = torch.from_numpy(vals).to(DEV).requires_grad_(True)
        got = conv.aggregate(xg, idx_d, N, _graph=graph)
        gg, = torch.autograd.grad((got * cot.to(DEV)).sum(), [xg], retain_graph=True)
        g1, = torch.autograd.grad(got[:, :, k * F:(k + 1) * F].sum(), [xg])
        return got, gg, g1

    try:
        got, gg, g1 = nb_runs(monkeypatch, run)
    finally:
        graph.by_target.long_nodes = long_list
    check_close(got, want.detach().numpy(), None, None, what="block aggregate")
    check_close(gg, gw.numpy(), None, None, what="block aggregate grad", signed_sum=True)
    assert torch.equal(g1, w1), "arg of the max block differs from the oracle's (lowest edge position on ties)"
    graph.by_target.check()


@pytest.mark.parametrize("aggs,p", [(["min", "max"], 0.0), (["min", "max"], 0.5), (["sum", "mean", "max"], 0.0), (["sum", "mean", "max"], 0.5)])
def test_gr_block_layer_at_the_thresholds(aggs, p, monkeypatch):
    """The fused U + V + Z form (the layer call) on GR_CATALOGUE against the oracle with its float64 truth: output and dL/dx, forward and
    backward block kernels with dropout off and on, then the dV segment sum over the by-source grouping."""
    from mma_amd import functional as Fn
    from oracle import gr_oracle as G
    from oracle.dropout_rng import keep_mask
    from test_gr_gpu import conv_params, make_conv, to64
    T, F = 2, 8
    rng = np.random.default_rng(len(aggs) + int(p * 10))
    deg = gr_targets()
    N = len(deg)
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, len(dst))
    perm = rng.permutation(len(dst))
    ei = np.stack([src[perm], dst[perm]])
    E = ei.shape[1]
    conv = make_conv(aggs, ["identity", "attenuation"], towers=T, F=F, edge_dim=5)
    x = rng.standard_normal((N, conv.in_channels)).astype(np.float32)
    ea = rng.standard_normal((E, 5)).astype(np.float32)
    cot = rng.standard_normal((N, conv.out_channels)).astype(np.float32)
    seed = 0x5E6B10C
    conv.drop_override = Fn.DropoutSpec(p, seed=seed)
    keep = None
    if p > 0:
        Fw = conv.fused_width()
        keep = torch.from_numpy(keep_mask(seed, int(p * 256), 1, E, T * Fw)[0].reshape(E, T, Fw)[:, :, :F].astype(np.float32))
    xo = torch.from_numpy(x).requires_grad_(True)
    want = G.conv_forward(xo, torch.from_numpy(ei), torch.from_numpy(ea), conv_params(conv), conv.aggregators, conv.scalers,
                          conv.avg_deg, T, False, keep, p)
    gw, = torch.autograd.grad((want * torch.from_numpy(cot)).sum(), [xo])
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w64 = G.conv_forward(x64, torch.from_numpy(ei), torch.from_numpy(ea).double(), to64(conv_params(conv)), conv.aggregators,
                         conv.scalers, conv.avg_deg, T, False, keep, p)
    g64, = torch.autograd.grad((w64 * torch.from_numpy(cot).double()).sum(), [x64])
    eig = torch.from_numpy(ei).to(DEV)
    graph = Fn.gr_graph(eig, N)                      # the cached graph the layer call uses for this edge_index
    long_list = graph.by_target.long_nodes

    def run(with_list):
        graph.by_target.long_nodes = long_list if with_list else None
        xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
        got = conv(xg, eig, torch.from_numpy(ea).to(DEV))
        gg, = torch.autograd.grad((got * torch.from_numpy(cot).to(DEV)).sum(), [xg])
        return got, gg

    try:
        got, gg = nb_runs(monkeypatch, run)
    finally:
        graph.by_target.long_nodes = long_list
    check_close(got, want.detach().numpy(), None, None, what="block layer out", signed_sum=True, truth=w64.detach().numpy())
    check_close(gg, gw.numpy(), None, None, what="block layer gx", signed_sum=True, truth=g64.numpy())
    graph.by_target.check()


# ---- C. the tall Linear past 4096 outputs ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padded_grad", [False, True])
def test_linear_tall_past_4096_outputs(padded_grad):
    """dense.linear_tall with fin + 1 <= 64 (the narrow reduction widths) and fout = 4224 > 4096, where the narrow-K kernel does not take
    the product: the padded A operand must stay 128 wide for the general kernel.  Forward, dL/dx, dW and db against float64 at the bars of
    test_gemm_gpu.py::test_linear_tall_on_the_bf16x3_kernels."""
    from mma_amd import dense
    N, fin, fout = 32768, 50, 4224
    rng = np.random.default_rng(4224)
    x = torch.from_numpy(rng.standard_normal((N, fin)).astype(np.float32)).to(DEV).requires_grad_(True)
    w = torch.from_numpy((rng.standard_normal((fout, fin)) * 0.1).astype(np.float32)).to(DEV).requires_grad_(True)
    b = torch.from_numpy(rng.standard_normal(fout).astype(np.float32)).to(DEV).requires_grad_(True)
    assert dense.linear_x3_ok(x, w)
    y = dense.linear_tall(x, w, b)
    assert y.shape == (N, fout)
    cot_np = rng.standard_normal((N, fout)).astype(np.float32)
    if padded_grad:
        cot = dense.padded_empty(N, fout, DEV)
        cot.copy_(torch.from_numpy(cot_np))
    else:
        cot = torch.from_numpy(cot_np).to(DEV)
    got = torch.autograd.grad(y, [x, w, b], grad_outputs=cot)
    xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    yd = torch.nn.functional.linear(xd, wd, bd)
    ref = torch.autograd.grad(yd, [xd, wd, bd], grad_outputs=torch.from_numpy(cot_np).double().to(DEV))
    scale = xd.detach().abs() @ wd.detach().abs().t() + bd.detach().abs()
    assert ((y.double() - yd).abs() / scale).max().item() < 5e-7
    for g_, r_ in zip(got, ref):
        assert g_.shape == r_.shape
        assert (g_.double() - r_).abs().max().item() <= 2e-6 * r_.abs().max().item() + 1e-6 * N ** 0.5
