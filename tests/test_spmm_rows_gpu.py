"""K5 (the CSR SpMM) and K7 (the halo row kernels) of spmm_rows.hip at the boundaries of their dispatch, on row layouts built on purpose:

- mma_csr_spmm_items through the SpmmGraph plans, forward and transposed: items of SPMM_GROUP_BELOW = 64 edges and more run one per
  wavefront, shorter ones one per lane group; rows above SPMM_CHUNK = 512 edges are cut into hub chunks whose partial sums the finalize
  kernel adds in slot order; the width C picks the float4 or the scalar path, the lanes per row (lpr), the column chunks (blockIdx.y,
  from C > 256 / C > 64 on) and the groups per wavefront (gpw; gpw == 1 and chunks > 1 have no group pass and no one-launch form);
- mma_csr_spmm / mma_csr_spmm_rm outside the segment-sum gate: K > 1, edge weights, bias, widths the block kernel does not take;
- mma_pack_rows, mma_unpack_add_rows and mma_unpack_add_rows_csr, bit for bit.

Every output buffer starts NaN-filled; direct ABI calls write into a buffer wider than the payload whose pad columns must stay NaN.
Accuracy is golden_util.check_close against the fp32 CPU product with a float64 truth; everything else is bit equality."""
import numpy as np
import pytest
import torch

from golden_util import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CHUNK, GROUP_BELOW = 512, 64                       # graph.py: SPMM_CHUNK, SPMM_GROUP_BELOW
MAX_GRID = 256 * 8                                 # common.h: kMaxGrid (the group pass and the row kernels stride beyond 4 * kMaxGrid)
NAN = float("nan")

V4_WIDTHS = [4, 8, 12, 16, 64, 128, 132, 256, 260, 516]
SCALAR_WIDTHS = [1, 2, 3, 5, 7, 33, 64, 65, 130]
# every degree the issue names, each in a known row: 0 .. 9 (the group pass's 4-edge unroll and its tail), SPMM_GROUP_BELOW - 1 / +0 / +1,
# 127 .. 129 (two wavefront loads), SPMM_CHUNK - 1 / +0 / +1 (no hub / hub of 2), 1024, 1025, 1537 (hubs of 2, 3, 4 slots, last chunk
# of one edge) and one row of 5 000
MAIN_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025, 1537, 5000, 0, 6, 2, 0, 1, 10, 3]


def path_of(C, aligned=True):
    """(vec, lpr_log, chunks, gpw) that the launchers of spmm_rows.hip derive from the width (aligned: pitches % 4 == 0, bases % 16 == 0)."""
    vec = 4 if (aligned and C % 4 == 0) else 1
    per_row = -(-C // vec)
    lpr_log = 0
    while (1 << lpr_log) < per_row and lpr_log < 6:
        lpr_log += 1
    return vec, lpr_log, -(-per_row // (1 << lpr_log)), 64 >> lpr_log


def path_id(C, aligned=True):
    return "C%d-vec%d-lpr_log%d-chunks%d-gpw%d" % ((C,) + path_of(C, aligned))


def widths(v4, scalar):
    """(C, aligned) cases: the float4 widths as they are; the scalar widths, of which a multiple of 4 (C = 64: the widest scalar row of
    one column chunk) is demoted by a B pitch of C + 1."""
    return [pytest.param(C, True, id=path_id(C)) for C in v4] + \
           [pytest.param(C, C % 4 != 0, id=path_id(C, False) + ("-demoted" if C % 4 == 0 else "")) for C in scalar]


def operand(Bh, aligned):
    """B on the device; not `aligned`: as a view of a buffer with one more column (a pitch that is no multiple of 4)."""
    if not Bh.shape[0]:
        return torch.empty((1, Bh.shape[1] + (0 if aligned else 1)), device=DEV)[:0, :Bh.shape[1]]
    return dev(Bh) if aligned else padded(Bh, 1)[0]


def expected_plan(deg):
    """(n_items, n_wave_items, n_slots, n_hubs) of a CSR with these row degrees, from the definition: a row of more than CHUNK edges is
    cut into ceil(deg / CHUNK) chunks with a slot each; items of GROUP_BELOW edges and more run one per wavefront."""
    deg = np.asarray(deg, np.int64)
    nch = np.maximum(1, -(-deg // CHUNK))
    last = deg - (nch - 1) * CHUNK
    n_wave = int(((nch - 1) * (CHUNK >= GROUP_BELOW) + (last >= GROUP_BELOW)).sum())
    return int(nch.sum()), n_wave, int(nch[nch > 1].sum()), int((nch > 1).sum())


def weights(rng, n):
    """Real edge weights: both signs and a few exact zeros."""
    v = rng.standard_normal(n).astype(np.float32)
    v[rng.random(n) < 0.03] = 0.0
    return v


def coo(deg, n_cols, rng, weighted):
    """(row, col, val) of a matrix with these row degrees and no element stored twice (a coalesced matrix, as SpmmGraph is given one:
    the same value added hundreds of times would round the same way every time, which no reference formed from the summed value does).
    A row's columns are a run of a random column order from a random start, so deg <= n_cols rows have distinct columns."""
    deg = np.asarray(deg, np.int64)
    assert not len(deg) or deg.max() <= n_cols
    row = np.repeat(np.arange(len(deg)), deg)
    within = np.arange(len(row)) - (np.cumsum(deg) - deg)[row]
    col = rng.permutation(n_cols)[(rng.integers(0, n_cols, len(deg))[row] + within) % n_cols]
    return row, col, (weights(rng, len(row)) if weighted else None)


def main_degrees(n_rows, rng):
    """MAIN_DEGREES in rows 0 .. 28, then short rows (0 .. 6 edges) up to n_rows."""
    return np.concatenate([MAIN_DEGREES, rng.integers(0, 7, n_rows - len(MAIN_DEGREES))]).astype(np.int64)


def product(row, col, val, shape, B, bias, dtype, K=1):
    """sum_k A @ B[k] + bias on the CPU in `dtype`; B: (K * shape[1], C).  torch.sparse.mm on the coalesced matrix, K > 1 in the form the
    layer being reproduced computes it (layers.py:861-865, as tests/test_nc_gpu.py::test_spmm_matches_torch_sparse): ONE product with the
    K-times column-stacked matrix, so that a row is one sum of K * deg terms in the reference as it is in the kernel and the reference's
    own fp32 noise - what check_close scales its bar with - is that of a sum of this length.  (Measured once with K separate products
    added up, whose 5 000-term sums are ~4x less noisy than one 40 000-term sum: at K = 8, C = 256, unit weights + bias one element
    of 7 424 - the 5 000-edge row, 115.213 against 115.218 - was 0.0052 off at a bar of 0.00512; every other case met that bar too.)"""
    C = B.shape[1]
    out = torch.zeros((shape[0], C), dtype=dtype)
    if len(row) and shape[0]:
        v = np.ones(len(row), np.float32) if val is None else val
        A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(v).to(dtype), shape).coalesce()
        out = out + torch.sparse.mm(A if K == 1 else torch.cat((A,) * K, 1), torch.from_numpy(B).to(dtype))
    if bias is not None:
        out = out + torch.from_numpy(bias).to(dtype)
    return out.numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(a, pad, offset=0):
    """A device copy of the 2-D array as a view (rows, width) of a buffer with row pitch width + pad that starts `offset` floats into its
    allocation; the pad columns hold NaN."""
    rows, width = a.shape
    flat = torch.full((rows * (width + pad) + offset,), NAN, device=DEV)
    view = flat[offset:].view(rows, width + pad)
    view[:, :width] = torch.from_numpy(a).to(DEV)
    return view[:, :width], view


def assert_pad_is_nan(full, width, what):
    assert bool(torch.isnan(full[:, width:]).all()), what + ": a pad column of the output was written"


class PlanSet:
    """One direction of a SpmmGraph: the arrays functional._spmm_call takes."""

    def __init__(self, sg, transposed):
        t = "t_" if transposed else ""
        self.rowptr, self.col, self.val = (getattr(sg, t + f) for f in ("rowptr", "col", "val"))
        self.items, self.hubs = getattr(sg, t + "items"), getattr(sg, t + "hubs")
        self.n_slots, self.n_wave_items = getattr(sg, t + "n_slots"), getattr(sg, t + "n_wave_items")
        self.n_rows, self.n_cols = (sg.n_cols, sg.n_rows) if transposed else (sg.n_rows, sg.n_cols)
        self.name = "transposed" if transposed else "forward"

    def plan(self):
        return self.items.shape[0], self.n_wave_items, self.n_slots, self.hubs.shape[0]

    def degrees(self):
        return np.diff(self.rowptr.cpu().numpy().astype(np.int64))


def run_items(s, B, bias, C):
    """functional._spmm_call (K = 1: mma_csr_spmm_items) into a NaN-filled (n_rows, C) output."""
    from mma_amd import functional as Fn
    out = torch.full((s.n_rows, C), NAN, device=DEV)
    Fn._spmm_call(s.rowptr, s.col, s.val, s.items, s.hubs, s.n_slots, B, s.n_cols, 1, bias, out, s.n_rows, C, s.n_wave_items)
    torch.cuda.synchronize()
    return out


def run_items_direct(s, B, bias, C, pad, what):
    """mma_csr_spmm_items through the ABI: output pitch C + pad, NaN-filled slot buffer; the pad columns must stay NaN."""
    from mma_amd._lib import call, stream_ptr
    full = torch.full((s.n_rows, C + pad), NAN, device=DEV)
    partial = torch.full((s.n_slots, C), NAN, device=DEV) if s.n_slots else None
    call("mma_csr_spmm_items", s.col, s.val, B, B.stride(0), bias, full, C + pad, s.items, s.items.shape[0], s.n_wave_items,
         s.hubs if s.n_slots else None, s.hubs.shape[0], partial, s.n_slots, C, stream_ptr())
    torch.cuda.synchronize()
    assert_pad_is_nan(full, C, what)
    return full[:, :C].contiguous()


def assert_empty_rows(got, deg, bias, what):
    """Degree-0 rows: exactly the bias, or exactly 0."""
    empty = torch.from_numpy(np.nonzero(deg == 0)[0]).to(got.device)
    rows = got[empty]
    want = torch.zeros_like(rows) if bias is None else bias.to(got.device).expand_as(rows)
    assert bool((rows == want).all()), what + ": a degree-0 row is not exactly " + ("0" if bias is None else "the bias")


def check_items(s, B, bias, C, want, truth, what, monkeypatch, aligned=True):
    """One direction of one plan: the call twice (same bits), the check_close bar, the degree-0 rows, the two-launch form against the
    one-launch form where both kinds of item exist in one column chunk, and the ABI call into a padded output (same bits)."""
    vec, lpr_log, chunks, gpw = path_of(C, aligned)
    what = "%s %s [%s items=%d wave=%d slots=%d hubs=%d]" % ((what, s.name, path_id(C, aligned)) + s.plan())
    got = run_items(s, B, bias, C)
    assert not bool(torch.isnan(got).any()), what + ": NaN left in the output (a row or column never written)"
    assert torch.equal(run_items(s, B, bias, C), got), what + ": second run differs"
    assert got.shape == want.shape
    if s.n_rows:
        check_close(got, want, None, None, what=what, signed_sum=True, truth=truth)
    assert_empty_rows(got, s.degrees(), bias, what)
    if chunks == 1 and gpw > 1 and 0 < s.n_wave_items < s.items.shape[0]:
        monkeypatch.setenv("MMA_SPMM_ONE_LAUNCH", "0")
        two = run_items(s, B, bias, C)
        monkeypatch.delenv("MMA_SPMM_ONE_LAUNCH")
        assert torch.equal(two, got), what + ": the two launches differ from the one launch"
    assert torch.equal(run_items_direct(s, B, bias, C, 4 if vec == 4 else 1, what), got), what + ": padded output differs"
    return got


def check_both_directions(row, col, val, n_rows, n_cols, C, rng, what, monkeypatch, deg=None, biases=(False, True), mirror=True,
                          aligned=True):
    """A @ B and A^T @ G on the plan of A (forward / transposed set) and, with `mirror`, on the plan of A^T (its transposed / forward set:
    the same two CSRs through the other half of the constructor - the same bits).  deg: the row degrees A was built with."""
    from mma_amd.graph import SpmmGraph
    sg = SpmmGraph(row, col, val, n_rows, n_cols, DEV)
    sets = {"A": [PlanSet(sg, False)], "At": [PlanSet(sg, True)]}
    if mirror:
        sgT = SpmmGraph(col, row, val, n_cols, n_rows, DEV)
        sets["A"].append(PlanSet(sgT, True))
        sets["At"].append(PlanSet(sgT, False))
    for s in sets["A"] + sets["At"]:
        d = s.degrees()
        assert s.plan() == expected_plan(d), "%s %s: plan %s, expected %s" % (what, s.name, s.plan(), expected_plan(d))
    if deg is not None:
        for s in sets["A"]:
            assert np.array_equal(s.degrees(), deg), what + ": the plan does not have the degrees the layout was built with"
    for (r, c, shape, key) in ((row, col, (n_rows, n_cols), "A"), (col, row, (n_cols, n_rows), "At")):
        Bh = rng.standard_normal((shape[1], C)).astype(np.float32)
        bh = rng.standard_normal(C).astype(np.float32)
        B = operand(Bh, aligned)
        for with_bias in biases:
            want = product(r, c, val, shape, Bh, bh if with_bias else None, torch.float32)
            truth = product(r, c, val, shape, Bh, bh if with_bias else None, torch.float64)
            outs = [check_items(s, B, dev(bh) if with_bias else None, C, want, truth,
                                "%s %s%s" % (what, "weighted" if val is not None else "unit", " +bias" if with_bias else ""), monkeypatch, aligned)
                    for s in sets[key]]
            assert all(torch.equal(o, outs[0]) for o in outs), what + ": the plan of A and the plan of A^T give other bits for the same CSR"
    return sg


# ---- A. mma_csr_spmm_items through SpmmGraph --------------------------------------------------------------------------------------------

SHAPES = {"square": (5101, 5101), "tall": (6029, 5003), "wide": (len(MAIN_DEGREES), 6007)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("C,aligned", widths(V4_WIDTHS, SCALAR_WIDTHS))
def test_items_at_the_thresholds(C, aligned, shape, monkeypatch):
    """MAIN_DEGREES (then short rows; n_rows odd: not a multiple of 4 nor of any 64 >> lpr_log) at every width, square / more rows than
    columns / fewer, unit and real weights, with and without bias, forward and transposed."""
    n_rows, n_cols = SHAPES[shape]
    rng = np.random.default_rng(C * 7 + len(shape))
    deg = main_degrees(n_rows, rng)
    assert n_rows % 2 and expected_plan(deg) == (len(deg) + 1 + 1 + 2 + 3 + 9, 7 + 1 + 2 + 2 + 3 + 10, 2 + 2 + 3 + 4 + 10, 5)
    for weighted in (False, True):
        row, col, val = coo(deg, n_cols, rng, weighted)
        sg = check_both_directions(row, col, val, n_rows, n_cols, C, rng, "main %s" % shape, monkeypatch, deg=deg, aligned=aligned)
        assert (sg.val is not None) == weighted and (sg.t_val is not None) == weighted


LAYOUTS = {
    "all_short": lambda rng: np.concatenate([rng.integers(0, GROUP_BELOW, 98), [GROUP_BELOW - 1, 0, GROUP_BELOW - 1]]),
    "all_long": lambda rng: np.array([64, 65, 127, 200, 512, 576, 1024, 1100, 64, 300, 64]),
    "all_empty": lambda rng: np.zeros(37, np.int64),
    "odd_rows": lambda rng: np.concatenate([rng.integers(0, 131, 100), [700]]),
    "no_rows": lambda rng: np.zeros(0, np.int64),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C,aligned", widths([4, 16, 132, 260], [7, 65]))
def test_items_layouts(C, aligned, layout, monkeypatch):
    """Plans with no per-wavefront item, with nothing but per-wavefront items, with no edge at all, with 101 rows, and with no row."""
    rng = np.random.default_rng(C + len(layout))
    deg = LAYOUTS[layout](rng).astype(np.int64)
    n_items, n_wave, n_slots, n_hubs = expected_plan(deg)
    if layout == "all_short":
        assert n_wave == 0 and n_slots == 0 and n_items == 101
    if layout == "all_long":
        assert n_wave == n_items and n_hubs == 3 and n_slots == 7
    if layout == "all_empty":
        assert (n_items, n_wave, n_slots, n_hubs) == (37, 0, 0, 0)
    if layout == "odd_rows":
        assert len(deg) % 4 and len(deg) % 2 and 0 < n_wave < n_items and n_hubs == 1
    if layout == "no_rows":
        assert n_items == 0
    row, col, val = coo(deg, 1103, rng, True)
    check_both_directions(row, col, val, len(deg), 1103, C, rng, layout, monkeypatch, deg=deg, aligned=aligned)


@pytest.mark.parametrize("how", ["pitch17", "offset1"])
def test_items_c16_demoted_to_scalar(how, monkeypatch):
    """C = 16 would take the float4 path; a B pitch of 17 floats, or a B base one float into its allocation, must demote it to the scalar
    path (lpr_log 4, gpw 4) instead of issuing misaligned 16-byte loads."""
    from mma_amd.graph import SpmmGraph
    C = 16
    assert path_of(C) == (4, 2, 1, 16) and path_of(C, aligned=False) == (1, 4, 1, 4)
    rng = np.random.default_rng(len(how))
    deg = np.array(MAIN_DEGREES, np.int64)
    n_rows, n_cols = len(deg), 5003
    row, col, val = coo(deg, n_cols, rng, True)
    sg = SpmmGraph(row, col, val, n_rows, n_cols, DEV)
    for transposed in (False, True):
        s = PlanSet(sg, transposed)
        r, c, shape = (col, row, (n_cols, n_rows)) if transposed else (row, col, (n_rows, n_cols))
        Bh = rng.standard_normal((shape[1], C)).astype(np.float32)
        bh = rng.standard_normal(C).astype(np.float32)
        B, full = padded(Bh, 1, 0) if how == "pitch17" else padded(Bh, 0, 1)
        assert B.stride(0) == (17 if how == "pitch17" else 16) and (B.data_ptr() % 16 == 0) == (how == "pitch17")
        want, truth = (product(r, c, val, shape, Bh, bh, dt) for dt in (torch.float32, torch.float64))
        what = "demoted by %s %s [%s]" % (how, s.name, path_id(C, aligned=False))
        got = run_items_direct(s, B, dev(bh), C, 4, what)
        assert torch.equal(run_items_direct(s, B, dev(bh), C, 4, what), got), what + ": second run differs"
        check_close(got, want, None, None, what=what, signed_sum=True, truth=truth)
        assert_empty_rows(got, s.degrees(), dev(bh), what)
        check_items(s, B, dev(bh), C, want, truth, "demoted by " + how, monkeypatch, aligned=False)      # functional._spmm_call on the view


@pytest.mark.parametrize("C,aligned", widths([16, 64], [7]))
def test_items_feature_matrix_like(C, aligned, monkeypatch):
    """The sparse-feature first layer: a weighted 2 708 x 1 433 matrix at ~1.3 % density; a few words occur in more than 512 documents, so
    the transposed plan (the weight gradient's) has weighted hub chunks and their slot sums."""
    rng = np.random.default_rng(C)
    n_rows, n_cols = 2708, 1433
    p = np.full(n_cols, 0.0125)
    p[[3, 700, 1432]] = (0.25, 0.4, 0.22)
    row, col = np.nonzero(rng.random((n_rows, n_cols)) < p[None, :])
    val = weights(rng, len(row))
    assert 0.012 < len(row) / (n_rows * n_cols) < 0.014
    sg = check_both_directions(row, col, val, n_rows, n_cols, C, rng, "feature matrix", monkeypatch, mirror=False, aligned=aligned)
    assert sg.n_slots == 0 and sg.t_hubs.shape[0] == 3 and sg.t_n_slots >= 6 and sg.t_val is not None
    assert 0 < sg.t_n_wave_items < sg.t_items.shape[0]


def interleave(rng, *parts):
    deg = np.concatenate(parts)
    return deg[rng.permutation(len(deg))]


@pytest.mark.parametrize("kind", ["wave", "group", "both"])
def test_items_grid_stride(kind, monkeypatch):
    """More work than one round of workgroups: more than 4 * kMaxGrid per-wavefront items (kMaxGrid workgroups of four wavefronts) at
    C = 16; more than 4 * kMaxGrid workgroups of short items at C = 128 (gpw = 2: eight items per workgroup); and both in one launch."""
    rng = np.random.default_rng(len(kind))
    n_long, n_short = 4 * MAX_GRID + 77, 4 * MAX_GRID * 8 + 333
    long_rows, short_rows = rng.integers(64, 71, n_long), rng.integers(0, 6, n_short)
    C, deg = {"wave": (16, long_rows), "group": (128, short_rows), "both": (128, interleave(rng, long_rows, short_rows))}[kind]
    vec, lpr_log, chunks, gpw = path_of(C)
    n_items, n_wave, n_slots, n_hubs = expected_plan(deg)
    if kind != "group":
        assert (n_wave + 3) // 4 > MAX_GRID, "per-wavefront pass inside one round"
    if kind != "wave":
        assert (n_items - n_wave + 4 * gpw - 1) // (4 * gpw) > 4 * MAX_GRID, "group pass inside one round"
    n_cols = 4096
    row, col, val = coo(deg, n_cols, rng, True)
    check_both_directions(row, col, val, len(deg), n_cols, C, rng, "grid stride %s" % kind, monkeypatch, deg=deg, biases=(True,), mirror=False)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("C,aligned", widths([16, 260], [7]))
def test_csr_spmm_wrapper_equals_the_direct_calls(C, aligned, K, monkeypatch):
    """functional.csr_spmm on the plan: its output is the direct call's, its dL/dB the transposed direct call's (the same for every
    k-block), its bias gradient dense.col_sum of the cotangent - bit for bit."""
    from mma_amd import dense, functional as Fn
    from mma_amd.graph import SpmmGraph
    rng = np.random.default_rng(C + K)
    deg = np.array(MAIN_DEGREES, np.int64)
    n_rows, n_cols = len(deg), 5003
    row, col, val = coo(deg, n_cols, rng, True)
    sg = SpmmGraph(row, col, val, n_rows, n_cols, DEV)
    Bh, bh = rng.standard_normal((K * n_cols, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    g = dev(rng.standard_normal((n_rows, C)).astype(np.float32))
    B, bias = dev(Bh).requires_grad_(True), dev(bh).requires_grad_(True)
    out = Fn.csr_spmm(B, bias, sg, K)
    gB, gb = torch.autograd.grad(out, [B, bias], grad_outputs=g)
    if K == 1:
        direct = run_items(PlanSet(sg, False), B.detach(), bias.detach(), C)
    else:
        direct = spmm_rows(sg.rowptr, sg.col, sg.val, B.detach(), n_cols, K, bias.detach(), n_rows, C, 0, "wrapper")
    assert torch.equal(out.detach(), direct), "csr_spmm differs from the direct call"
    want, truth = (product(row, col, val, (n_rows, n_cols), Bh, bh, dt, K) for dt in (torch.float32, torch.float64))
    check_close(out, want, None, None, what="csr_spmm K=%d %s" % (K, path_id(C)), signed_sum=True, truth=truth)
    gB1 = run_items(PlanSet(sg, True), g, None, C)
    assert gB.shape == (K * n_cols, C) and all(torch.equal(gB[k * n_cols:(k + 1) * n_cols], gB1) for k in range(K)), "dL/dB"
    assert torch.equal(gb, dense.col_sum(g)), "bias gradient differs from dense.col_sum"


# ---- B. mma_csr_spmm / mma_csr_spmm_rm outside the segment-sum gate -----------------------------------------------------------------------

def segsum_gate(C, K, val, bias, aligned=True):
    """csr_spmm_impl hands K = 1, unit weights, no bias at 32 <= C <= 1024 float4 widths to the block segment sum (its own test module)."""
    return K == 1 and val is None and bias is None and aligned and C % 4 == 0 and 32 <= C and 16 * C * 4 <= 64 * 1024


def spmm_rows(rowptr, col, val, B, rpb, K, bias, n_rows, C, pad, what, row_max=None):
    """mma_csr_spmm (mma_csr_spmm_rm with row_max) into a NaN-filled output of pitch C + pad."""
    from mma_amd._lib import call, stream_ptr
    full = torch.full((n_rows, C + pad), NAN, device=DEV)
    args = (rowptr, col, val, B, B.stride(0), rpb, K, bias, full, C + pad, n_rows, C)
    if row_max is None:
        call("mma_csr_spmm", *args, stream_ptr())
    else:
        call("mma_csr_spmm_rm", *args, row_max, stream_ptr())
    torch.cuda.synchronize()
    assert_pad_is_nan(full, C, what)
    return full[:, :C].contiguous()


def check_spmm_rows(deg, n_cols, C, aligned, K, rng, what):
    """Every (weights, bias) combination that stays outside the segment-sum gate: the bar, a second run, the _rm form and its row maxima."""
    vec = path_of(C, aligned)[0]
    pad = 4 if vec == 4 else 1
    n_rows = len(deg)
    ran = 0
    for weighted, with_bias in ((True, True), (True, False), (False, True), (False, False)):
        row, col, val = coo(deg, n_cols, rng, weighted)
        Bh, bh = rng.standard_normal((K * n_cols, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        bias = bh if with_bias else None
        if segsum_gate(C, K, val, bias, aligned):
            continue
        ran += 1
        w = "%s K=%d %s%s [%s]" % (what, K, "weighted" if weighted else "unit", " +bias" if with_bias else "", path_id(C, aligned))
        rowptr = dev(np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))
        args = (rowptr, dev(col.astype(np.int32)), dev(val), operand(Bh, aligned), n_cols, K, dev(bias), n_rows, C, pad, w)
        got = spmm_rows(*args)
        assert not bool(torch.isnan(got).any()), w + ": NaN left in the output"
        assert torch.equal(spmm_rows(*args), got), w + ": second run differs"
        want, truth = (product(row, col, val, (n_rows, n_cols), Bh, bias, dt, K) for dt in (torch.float32, torch.float64))
        check_close(got, want, None, None, what=w, signed_sum=True, truth=truth)
        assert_empty_rows(got, deg, dev(bias), w)
        rm = torch.zeros(n_rows, device=DEV)
        assert torch.equal(spmm_rows(*args, row_max=rm), got), w + ": mma_csr_spmm_rm output differs from mma_csr_spmm"
        assert torch.equal(rm, got.abs().amax(1)), w + ": row maxima are not max |row|"
        zero_rows = (got == 0).all(1)
        assert bool((rm[zero_rows] == 0).all()) and (with_bias or int(zero_rows.sum()) >= int((deg == 0).sum()) > 0), w + ": all-zero rows"
    assert ran >= 3


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("C,aligned", widths(V4_WIDTHS, SCALAR_WIDTHS))
def test_spmm_rows_at_the_thresholds(C, aligned, K):
    """The wave-per-row kernel on MAIN_DEGREES (the hub rows are one wavefront's walk here) with K column-stacked blocks of B."""
    check_spmm_rows(np.array(MAIN_DEGREES, np.int64), 5003, C, aligned, K, np.random.default_rng(C * 10 + K), "rows")


@pytest.mark.parametrize("C,aligned", widths([16, 260], [7]))
def test_spmm_rows_grid_stride(C, aligned):
    """More rows than kMaxGrid workgroups of four wavefronts take in one round."""
    rng = np.random.default_rng(C)
    deg = interleave(rng, rng.integers(0, 10, 4 * MAX_GRID + 301), np.array([64, 65, 129, 600]))
    assert (len(deg) + 3) // 4 > MAX_GRID
    check_spmm_rows(deg, 1000, C, aligned, 2, rng, "rows grid stride")


# ---- C. the halo row kernels, bit for bit -------------------------------------------------------------------------------------------------

ROW_WIDTHS = [1, 3, 4, 7, 16, 128, 130]
PITCHES = ["tight", "mult4", "odd", "offset1"]     # pitch == width / a larger multiple of 4 / not a multiple of 4 / base one float in


def pitch_of(W, pitch):
    pad = {"tight": 0, "mult4": -(-W // 4) * 4 + 4 - W, "odd": -(-W // 4) * 4 + 5 - W, "offset1": -(-W // 4) * 4 + 4 - W}[pitch]
    return pad, int(pitch == "offset1")


def row_counts(W):
    return [0, 1, 257] + ([70000] if W == 128 else [])                # 70 000 rows of 32 float4 (or 128 floats): beyond 4 * kMaxGrid workgroups


def buffers(rng, rows, W, pitch):
    """(host array (rows, W), device view of it inside a NaN-padded buffer, the whole buffer (rows, pitch))."""
    a = rng.standard_normal((rows, W)).astype(np.float32)
    pad, offset = pitch_of(W, pitch)
    view, full = padded(a, pad, offset)
    return a, view, full


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def rows_call(name, src, idx, n, dst, W):
    from mma_amd._lib import call, stream_ptr
    call(name, src, src.stride(0), idx, n, dst, dst.stride(0), W, stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("W", ROW_WIDTHS)
def test_pack_rows(W, pitch):
    """dst[t] = src[idx[t]] (idx repeats rows); the pad columns of dst and the rows past n_idx keep their NaN."""
    rng = np.random.default_rng(W * 10 + len(pitch))
    for n in row_counts(W):
        if n == 70000:
            assert (n * (W // 4 if W % 4 == 0 and pitch in ("tight", "mult4") else W) + 255) // 256 > 4 * MAX_GRID
        src_h, src, _ = buffers(rng, 300, W, pitch)
        idx = rng.integers(0, 300, n).astype(np.int32)
        pad, offset = pitch_of(W, pitch)
        dst, full = padded(np.full((n + 3, W), np.nan, np.float32), pad, offset)
        rows_call("mma_pack_rows", src, dev(idx), n, dst, W)
        want = np.full((n + 3, W + pad), np.nan, np.float32)
        want[:n, :W] = src_h[idx]
        assert np.array_equal(bits(full), want.view(np.int32)), "pack W=%d %s n_idx=%d" % (W, pitch, n)


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("W", ROW_WIDTHS)
def test_unpack_add_rows(W, pitch):
    """dst[idx[t]] += src[t] with unique idx: one fp32 addition per element, rows not named and pad columns unchanged."""
    rng = np.random.default_rng(W * 10 + len(pitch) + 1)
    for n in row_counts(W):
        src_h, src, _ = buffers(rng, max(n, 1), W, pitch)
        dst_h, dst, full = buffers(rng, n + 50, W, pitch)
        idx = rng.permutation(n + 50)[:n].astype(np.int32)
        rows_call("mma_unpack_add_rows", src, dev(idx), n, dst, W)
        want = torch.from_numpy(dst_h).index_add(0, torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(src_h[:n])).numpy()
        assert np.array_equal(bits(full[:, :W]), want.view(np.int32)), "unpack-add W=%d %s n_idx=%d" % (W, pitch, n)
        assert_pad_is_nan(full, W, "unpack-add W=%d %s n_idx=%d" % (W, pitch, n))


class UnpackPlan:
    """What HaloPlan.build_unpack reads of a HaloPlan (whose constructor needs a process group)."""

    def __init__(self, send_idx, n_own, plan_device=None):
        from mma_amd.sharded import HaloPlan
        self.send_idx, self.n_own, self.plan_device = np.asarray(send_idx, np.int64), n_own, plan_device
        HaloPlan.build_unpack(self)

    def lists(self):
        return self.unpack_rows, self.unpack_segptr, self.unpack_pos


def send_list(rng, n_rows, n_own):
    """send_idx of a rank whose rows are read by up to seven peers: n_rows distinct local rows occurring 1, 2, 3 and 7 times, peer by peer
    (a peer's rows ascend, as HaloPlan's do)."""
    rows = np.sort(rng.permutation(n_own)[:n_rows])
    times = np.array([1, 2, 3, 7])[rng.integers(0, 4, n_rows)]
    times[:min(4, n_rows)] = [1, 2, 3, 7][:min(4, n_rows)]
    parts = [rows[times > p] for p in range(7)]
    return (np.concatenate(parts) if n_rows else np.zeros(0, np.int64)), times


def unpack_csr_reference(dst, src, rows, segptr, pos):
    """d = dst[row]; for q in pos[seg]: d = d + src[q] - in that order, fp32 (vectorised over the rows by position in the segment)."""
    out = dst.copy()
    cnt = np.diff(segptr)
    for t in range(int(cnt.max()) if len(cnt) else 0):
        sel = np.nonzero(cnt > t)[0]
        out[rows[sel]] = out[rows[sel]] + src[pos[segptr[sel] + t]]
    return out


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("W", ROW_WIDTHS)
def test_unpack_add_rows_csr(W, pitch):
    """The reverse halo exchange in one launch: every row named once, its received copies added in the order of `pos` - with the lists of
    HaloPlan.build_unpack (host and device builders: the same lists) and with a hand-made non-ascending pos; twice; bit for bit."""
    from mma_amd._lib import call, stream_ptr
    rng = np.random.default_rng(W * 10 + len(pitch) + 2)
    for n in row_counts(W):
        n_own = n + 40
        send_idx, times = send_list(rng, n, n_own)
        plan = UnpackPlan(send_idx, n_own)
        rows, segptr, pos = plan.lists()
        assert len(rows) == n and np.array_equal(np.diff(segptr), times) and (n < 4 or set(times) == {1, 2, 3, 7})
        if torch.cuda.is_available():
            for a, b in zip(UnpackPlan(send_idx, n_own, torch.device(DEV)).lists(), plan.lists()):
                assert a.dtype == b.dtype and np.array_equal(a, b), "device-built unpack lists differ from the host-built ones"
        shuffled = pos.copy()
        for t in range(len(rows)):
            shuffled[segptr[t]:segptr[t + 1]] = pos[segptr[t]:segptr[t + 1]][::-1]
        assert n < 2 or not np.array_equal(shuffled, pos)
        src_h, src, _ = buffers(rng, max(len(send_idx), 1), W, pitch)
        for order in (pos, shuffled):
            results = []
            dst_h = rng.standard_normal((n_own, W)).astype(np.float32)
            for _ in range(2):
                pad, offset = pitch_of(W, pitch)
                dst, full = padded(dst_h, pad, offset)
                call("mma_unpack_add_rows_csr", src, src.stride(0), dev(rows.astype(np.int32)), dev(segptr.astype(np.int32)),
                     dev(order.astype(np.int32)), n, dst, dst.stride(0), W, stream_ptr())
                torch.cuda.synchronize()
                assert_pad_is_nan(full, W, "unpack-add csr W=%d %s n=%d" % (W, pitch, n))
                results.append(bits(full[:, :W]))
            want = unpack_csr_reference(dst_h, src_h, rows, segptr, order)
            assert np.array_equal(results[0], want.view(np.int32)), "unpack-add csr W=%d %s n=%d: not the sequential fp32 sum" % (W, pitch, n)
            assert np.array_equal(results[1], results[0]), "unpack-add csr: second run differs"
