"""Dense pre/post transforms of the hot path.  Tall products run on the split-precision GEMMs of csrc/gemm_x3.hip (three fp16 x 2 or six
bf16 x 3 piece products per fp32 one): nn_form() / tn_form() are the ONE place where a shape meets its kernel, also for whoever must know the
answer ahead of the call (a pad width, a row-maxima buffer).  The rest are library GEMMs (rocBLAS / hipBLASLt fp32 MFMA), with one twist:

The weight gradients are (in, N) @ (N, out) products whose reduction dimension is the node count (1 M at C4) and whose
output is tiny (128 x 512): a single GEMM call leaves most of the 256 CUs idle (measured 49-75 TFLOP/s, and 3.4 TFLOP/s
for the (128,N)@(N,16) tail).  Splitting the reduction into ~N/8192 batches (strided-batched GEMM + a sum over the
batch) fills the chip: 140 TFLOP/s, 89 % of the fp32 MFMA peak (0.97 ms instead of 2.7 ms per mask-weight half)."""
from functools import partial

import torch

from . import _lib
from ._env import flag, integer
from ._lib import call, ptr, stream_ptr


def _span(name, nbytes=0, flops=0, mfma=None):
    from . import functional as Fn      # late: functional imports this module
    return Fn._span(name, nbytes, flops, mfma)

_ROWS_PER_BATCH = 8192
_MIN_ROWS_X3 = 4096
_MIN_COLS_TN = integer("MMA_MIN_COLS_TN", 1)
_MIN_ROWS_TN = integer("MMA_MIN_ROWS_TN", 1024)    # the TN kernel from here on (Cora's 2 708 rows: the library's 128 x 256 x 2708 TN
                                                   # product takes 22-25 us, a fifth of the layer replay)
_MIN_ROWS_F16X2 = 1 << 16    # the three-product forms that take their row maxima from outside want tall inputs
USE_F16X2 = True             # the three-product fp16 x 2 kernels where the shape allows, instead of the six-product bf16 x 3 ones
F16X2_K = (64, 96, 128)      # reduction widths of the whole-row three-product kernel (mma_gemm_f16x2_k)
PACK_K256 = flag("MMA_PACK_K256")     # 0: round 4's K = 256 forward (fp32 rows split per column group)
USE_NLP = flag("MMA_DX_NLP")          # round 4: the pipelined one-accumulator form (0: round 3's kernel)
TN_KA256 = flag("MMA_TN_KA256")       # 0: 128-column blocks of x, one launch each (round 3)
BF16_EPILOGUE = flag("MMA_BF16_EPILOGUE")      # a bf16 `out` of mm_into is written by the GEMM's own epilogue where the form has one (0: fp32
                                               # product + the mma_rows_to_bf16 pass everywhere)
_BF16_OUT_FORMS = ("f16x2_k", "f16x2_k256", "f16x2_k256p")      # the forms with a bf16-output twin (the `_h` entry points, ABI 39)


# ---- shape -> form: pure functions of integers and of the switches above, which they read when called (bench.py and the tests set them)
def _rows_form(K, N):
    """Row maxima from outside: N in {128, 256} with K % 128 == 0 is ONE pass over `a` on the pipelined one-accumulator kernel (also
    for N = 256 - hidden width 256, C5); other shapes one launch of the two-accumulator kernel per 128-column block."""
    return "f16x2_nlp" if USE_NLP and N in (128, 256) and K % 128 == 0 and K >= 256 else "f16x2_n128"


def nn_form(M, K, N, *, accumulate=False, row_max_known=False, out_ok=True, aligned=True, named=False):
    """The key of _NN_RUN that out (M,N) (+)= a (M,K) @ w (K,N) runs on.  row_max_known: the caller brings max |a[i,:]| along; out_ok:
    no `out` yet, or a GPU fp32 one with unit column stride; aligned: `a` is read in place (_gpu_f32(a, aligned=True)); named: the
    caller asked for these kernels by name (gemm_bf16x3) - no admission, never "lib"."""
    rows = USE_F16X2 and K > 128 and K % 64 == 0 and N % 128 == 0 and M >= _MIN_ROWS_F16X2
    if accumulate and row_max_known and not named and out_ok and aligned and rows and N <= 512:      # the dL/dx shape
        return _rows_form(K, N)
    # the six-product kernel takes K == 128 with any N, or any K % 128 == 0 with N <= 128 (accumulator tiles live in registers); a
    # product with both K > 128 and N > 128 (hidden width 256: C5) is run as N/128 column blocks of the second form
    if not named and not (M >= _MIN_ROWS_X3 and N % 32 == 0 and K % 128 == 0 and (K == 128 or N <= 128 or N % 128 == 0)
                          and (out_ok or not accumulate)):
        return "lib"
    if USE_F16X2 and not accumulate and out_ok:
        if K in F16X2_K and N % 128 == 0 and N <= 4096 and M >= _MIN_ROWS_X3:
            return "f16x2_k"
        if rows and N > 128:      # hidden width 256 (C5): does not fit the whole-row form; the row maxima cost one pass over `a`
            if K == 256 and N <= 4096:
                return "f16x2_k256p" if PACK_K256 else "f16x2_k256"
            return _rows_form(K, N)
    return "bf16x3" if K == 128 or N <= 128 else "bf16x3_blocks"


def f16x2_n128_ok(M, K, N):
    """Does rows_mm_add_ take a three-product kernel once it is given a's row maxima?  The producer of `a` asks: it has to leave them."""
    return nn_form(M, K, N, accumulate=True, row_max_known=True).startswith("f16x2")


def _tn_cols(form, KA):
    """Columns of x per launch: wider x (C5) goes in 128-column blocks, [r4] in 256-column ones on the three-product kernel (G read once)."""
    return KA if KA <= 128 else (256 if form == "f16x2_tn" and TN_KA256 and KA % 256 == 0 else 128)


def _tn_window_fits(M, KA, NC, pitch, batch=None):
    """The TN kernels address one split's row range through a 32-bit buffer window: (rows per split) x (row pitch) must stay < 2 GB.
    The library tells the number of splits through its workspace: one (KA, NC) tile per split and product."""
    n_ws = (_lib.query("mma_gemm_bf16x3_tn_workspace_floats", M, KA, NC) if batch is None else
            _lib.query("mma_gemm_bf16x3_tn_batched_workspace_floats", M, KA, NC, batch))
    splits = max(1, n_ws // ((batch or 1) * KA * NC))
    rows = -(-(-(-M // splits)) // 32) * 32
    return (rows + 32) * pitch * 4 < 2 ** 31


def tn_form(M, KA, NC, *, ldx, ldg, g_row_max_known=False, batch=None, named=False):
    """The key of _TN_RUN that x (M,KA)^T @ g (M,NC) runs on (row pitches ldx, ldg; batch=B: B such products over column blocks of the
    same rows in one launch, or what ONE of them takes).  Up to 128 x columns (any count: ragged tiles are guarded) or whole 128-column
    blocks; any g width (graph regression's odd-width Linears: 75 x 76; the 3- / 7-class output weights of node classification: the
    library's TN product takes 22 us on Cora, 80 us on PubMed).  Three products when the caller brings g's row maxima - a pass over
    the wide operand would cost what the form saves -, else six."""
    pitch = max(ldx, ldg)
    if (batch is not None and M >= _MIN_ROWS_X3 and 8 <= KA <= 128 and NC >= 32 and pitch < (1 << 24)
            and _tn_window_fits(M, KA, NC, pitch, batch)):
        return "bf16x3_tn_batched"
    if not named and not (M >= _MIN_ROWS_TN and (8 <= KA <= 128 or KA % 128 == 0) and NC >= _MIN_COLS_TN
                          and _tn_window_fits(M, min(KA, 128), NC, pitch)):
        return "lib"
    return "f16x2_tn" if USE_F16X2 and g_row_max_known and M >= _MIN_ROWS_F16X2 else "bf16x3_tn"


def _gpu_f32(*ts, unit_cols=False, aligned=False):
    """GPU fp32 tensors - unit_cols: matrices with unit column stride; aligned: and a row pitch of whole float4s from a 16-byte base."""
    return all(t.is_cuda and t.dtype == torch.float32 and (not (unit_cols or aligned) or t.stride(1) == 1)
               and (not aligned or (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)) for t in ts)


# ---- form -> runner: (a, w, out, accumulate, row_max, box) with `out` allocated; each states its span name and mfma kind ------------
def _gemm_span(name, mfma, M, K, N, accumulate=False, c_bytes=4):
    """A in once (algorithmic: column blocks re-read it; B is 0.5 MB), C out - and in, when accumulating.  TN: x and g in once.
    c_bytes: 2 for a bf16 C."""
    return _span(name, nbytes=M * (4 * K + c_bytes * (2 if accumulate else 1) * N), flops=2 * M * K * N, mfma=mfma)


def _c_suffix(out):
    """"" / "_h": the entry point for the dtype of C, and the size of its elements."""
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("the three-product column-group GEMMs write float32 or bfloat16, but got %r" % (out.dtype,))
    return ("", 4) if out.dtype == torch.float32 else ("_h", 2)


def _row_max(a, box, fill=True):
    """(M,) max |a[i,:]| for a form that was not given them (fill=False: its own kernel fills the buffer); `box` hands them on."""
    rm = row_absmax(a) if fill else torch.empty((a.shape[0],), device=a.device, dtype=torch.float32)
    if box is not None:
        box.append(rm)
    return rm


def row_absmax(a):
    """max |a[i,:]| per row in one pass (mma_row_absmax); torch's a.abs().amax(1) is two kernels and a full-size temporary."""
    M, C = a.shape
    out = torch.empty((M,), device=a.device, dtype=torch.float32)
    if a.stride(1) != 1:
        a = a.contiguous()
    call("mma_row_absmax", ptr(a), a.stride(0) if M > 1 else C, M, C, ptr(out), stream_ptr())
    return out


def _split_f16x2(w, plain_lo=False):
    """w (K,N) fp32, any strides -> ((2,N,K) fp16 pieces of B^T scaled per column by a power of two that puts the column maximum
    into [2^14, 2^15), (N,) fp32 reciprocal scales): one launch (mma_split_f16x2).  plain_lo: the lo piece as it is, not times 2^11
    (the one-accumulator kernels)."""
    K, N = w.shape
    bt2 = torch.empty((2, N, K), device=w.device, dtype=torch.float16)
    cu = torch.empty((N,), device=w.device, dtype=torch.float32)
    call("mma_split_f16x2", ptr(w), w.stride(0), w.stride(1), K, N, ptr(bt2), ptr(cu), 1 if plain_lo else 0, stream_ptr())
    return bt2, cu


def gemm_f16x2(a, w, out=None, row_max_out=None, out_dtype=torch.float32):
    """a (M,K) @ w (K,N), K in F16X2_K, N % 128 == 0: the three-product form (fp16 hi/lo pieces, power-of-two row and column scales).
    row_max_out (M,): the kernel also leaves max |a[i,:]| there (it forms them for its row scales anyway).
    out_dtype torch.bfloat16 (or a bf16 `out`, whose dtype decides): the kernel's epilogue rounds its fp32 result to nearest even and
    stores bf16 (mma_gemm_f16x2_k_h) - the bits mma_rows_to_bf16 makes of the fp32 call's result, without that buffer or pass."""
    (M, K), N = a.shape, w.shape[1]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=out_dtype)
    h, c_bytes = _c_suffix(out)
    bt2, cu = _split_f16x2(w)
    with _gemm_span("gemm_x3_k128", "f16x3", M, K, N, c_bytes=c_bytes):
        call("mma_gemm_f16x2_k" + h, ptr(a), a.stride(0), ptr(bt2), ptr(cu), ptr(out), out.stride(0), ptr(row_max_out), M, N, K, stream_ptr())
    return out


def _run_f16x2_k256(a, w, out, accumulate, rm, box, packed=False):
    """K = 256 (C5 forward, N = 4096) with the whole 256-deep B slab resident per column group: A is read once per group through L2,
    not once per 128-column launch from HBM.  packed [r5]: A goes into fp16 fragment order first (one pass: row maxima, scale
    exponents, both pieces) and the 32 column groups stop re-splitting its rows; else the row maxima take a pass.
    A bf16 `out` is written by the kernel's epilogue (the `_h` entry points), as in gemm_f16x2."""
    (M, K), N = a.shape, w.shape[1]
    h, c_bytes = _c_suffix(out)
    rm = _row_max(a, box, fill=not packed)
    bt2, cu = _split_f16x2(w)
    if packed:
        ap = torch.empty((_lib.query("mma_pack_f16x2_k256_bytes", M),), device=a.device, dtype=torch.uint8)
        sce = torch.empty((M,), device=a.device, dtype=torch.int32)
        with _span("pack_f16x2", nbytes=8 * M * K, flops=0):
            call("mma_pack_f16x2_k256", ptr(a), a.stride(0), M, ptr(ap), ptr(sce), ptr(rm), stream_ptr())
    rows = (ptr(ap), ptr(sce)) if packed else (ptr(a), a.stride(0), ptr(rm))
    with _gemm_span("gemm_x3_persist", "f16x3", M, K, N, c_bytes=c_bytes):
        call(("mma_gemm_f16x2_k256p" if packed else "mma_gemm_f16x2_k256") + h, *rows, ptr(bt2), ptr(cu), ptr(out), out.stride(0), M, N, stream_ptr())
    return out


def _run_f16x2_rows(a, w, out, accumulate, rm, box, nlp=False):
    (M, K), N = a.shape, w.shape[1]
    if rm is None:
        rm = _row_max(a, box)
    bt2, cu = _split_f16x2(w, plain_lo=nlp)                              # (2, N, K), (N,)
    with _gemm_span("gemm_x3_acc" if accumulate else "gemm_x3_persist", "f16x3", M, K, N, accumulate):
        if nlp:
            call("mma_gemm_f16x2_nlp", ptr(a), a.stride(0), ptr(rm), ptr(bt2), ptr(cu), ptr(out), out.stride(0), M, N, K, accumulate, stream_ptr())
        # (walking A in row slabs that stay in the Infinity Cache between the column blocks was measured at C5's forward shape -
        # 32 blocks over a 1 GB A: 11.3 -> 11.2 ms, i.e. the kernel, not the re-reads of A, is what the product costs)
        for b in range(0 if nlp else N // 128):
            blk = bt2[:, 128 * b:128 * b + 128].contiguous() if N > 128 else bt2
            call("mma_gemm_f16x2_n128", ptr(a), a.stride(0), ptr(rm), ptr(blk), ptr(cu[128 * b:]), ptr(out[:, 128 * b:]), out.stride(0), M, K,
                 accumulate, stream_ptr())
    return out


def _run_bf16x3(a, w, out, accumulate, rm, box, blocks=False):
    (M, K), N = a.shape, w.shape[1]
    wt = w.t().contiguous()                                  # (N,K): B^T, k contiguous
    bt3 = torch.empty((3, N, K), device=a.device, dtype=torch.bfloat16)
    call("mma_split_bf16x3", ptr(wt), N * K, ptr(bt3), stream_ptr())
    with _gemm_span("gemm_x3_acc" if accumulate else "gemm_x3_k128" if K == 128 else "gemm_x3_persist", "bf16x6", M, K, N, accumulate):
        n = 128 if blocks else N                             # blocks: one launch per 128-column block of the output
        bt3 = bt3.view(3, N // n, n, K).permute(1, 0, 2, 3).contiguous()            # (N/n, 3, n, K): a block's own three pieces
        for b in range(N // n):
            call("mma_gemm_bf16x3", ptr(a), a.stride(0), ptr(bt3[b]), ptr(out[:, n * b:n * b + n]), out.stride(0), M, n, K, accumulate, stream_ptr())
    return out


def _run_lib(a, w, out, accumulate, rm, box):
    """The library GEMM.  A tall product into a new tensor is issued as a strided-batched GEMM over row blocks (w broadcast): rocBLAS
    then picks a kernel that runs 15-25 % faster than the single tall-skinny GEMM (C4: 94 -> 114 TFLOP/s forward, 105 -> 135
    TFLOP/s for g @ W^T)."""
    (M, K), N = a.shape, w.shape[1]
    B = M // _ROWS_PER_BATCH
    if out is not None and not accumulate:
        return torch.mm(a, w, out=out)
    if accumulate and B >= 4:
        return out.add_(_nn(a, w))
    with _gemm_span("lib_mm", "f32", M, K, N, accumulate):      # rocBLAS fp32
        if accumulate or B < 4:                 # accumulating: the library GEMM adds in its epilogue (beta = 1) - one launch, not two
            return out.addmm_(a, w) if accumulate else torch.mm(a, w)
        a = a.contiguous()
        n = B * _ROWS_PER_BATCH
        out = torch.empty((M, N), device=a.device, dtype=a.dtype)
        torch.bmm(a[:n].view(B, _ROWS_PER_BATCH, -1), w.unsqueeze(0).expand(B, -1, -1), out=out[:n].view(B, _ROWS_PER_BATCH, -1))
        if n < M:
            torch.mm(a[n:], w, out=out[n:])
        return out


_NN_RUN = {"f16x2_k": lambda a, w, out, accumulate, rm, box: gemm_f16x2(a, w, out, _row_max(a, box, fill=False) if box is not None else None),
           "f16x2_k256p": partial(_run_f16x2_k256, packed=True), "f16x2_k256": _run_f16x2_k256,
           "f16x2_nlp": partial(_run_f16x2_rows, nlp=True), "f16x2_n128": _run_f16x2_rows,
           "bf16x3": _run_bf16x3, "bf16x3_blocks": partial(_run_bf16x3, blocks=True), "lib": _run_lib}


def _nn(a, w, out=None, accumulate=False, row_max=None, box=None, named=False):
    """out (+)= a (M,K) @ w (K,N), no autograd: select the form, run it."""
    M, N = a.shape[0], w.shape[1]
    if M == 0 and out is not None:
        return out
    aligned = _gpu_f32(a, aligned=True)
    # a bf16 `out` (mm_into): the form is the one an fp32 `out` of the same shape takes
    out_h = out is not None and out.dtype == torch.bfloat16
    assert not (out_h and (accumulate or not out.is_cuda or out.shape != (M, N) or out.stride(1) != 1)), "a bf16 out: a GPU (M, N) matrix, never accumulated into"
    form = "lib" if not (named or _gpu_f32(a, w)) else nn_form(
        M, a.shape[1], N, accumulate=accumulate, row_max_known=row_max is not None,
        out_ok=out is None or out_h or _gpu_f32(out, unit_cols=True), aligned=aligned, named=named)
    dst = None
    if out_h and not (BF16_EPILOGUE and form in _BF16_OUT_FORMS):
        # no bf16 epilogue on this form (or the switch is off): the fp32 product as for an fp32 `out`, then the conversion pass - the
        # same function of the inputs on every shape
        dst, out = out, torch.empty((M, N), device=out.device, dtype=torch.float32)
    if form != "lib":
        a = a if aligned else a.contiguous()
        assert not accumulate if out is None else (out.shape == (M, N) and out.stride(1) == 1 and out.dtype in (torch.float32, torch.bfloat16))
        out = out if out is not None else torch.empty((M, N), device=a.device, dtype=torch.float32)
    res = _NN_RUN[form](a, w, out, accumulate, row_max, box)
    if dst is None:
        return res
    from . import functional as Fn      # late: functional imports this module
    return Fn.rows_to_bf16(res, dst)


def gemm_bf16x3(a, w, out=None, accumulate=False, row_max_box=None):
    """a (M,K) @ w (K,N) with fp32 accuracy on the split-precision kernels whatever M is (never the library): nn_form(named=True)
    picks among them.  `a` may be a row-strided view (a column block of a wider buffer); accumulate=True adds the product to `out`.
    row_max_box: a list that receives the (M,) row maxima of |a| when the form taken forms them anyway (the three-product ones)."""
    return _nn(a, w, out, accumulate, box=row_max_box, named=True)


def gemm_f16x2_n128(a, row_max, w, out, accumulate=False):
    """out (M,N) (+)= a (M,K) @ w (K,N), N a multiple of 128, on the three-product kernels that take the row maxima from outside
    (_rows_form picks); row_max (M,) >= max |a[i,:]| (0 for an all-zero row)."""
    return _NN_RUN[_rows_form(a.shape[1], w.shape[1])](a, w, out, accumulate, row_max, None)


def mm_into(a, w, out, row_max_box=None):
    """out[...] = a @ w (no autograd): the forward GEMMs of the sharded layer write row blocks of one buffer.  row_max_box: see
    gemm_bf16x3 (stays empty when the path taken does not form the row maxima of a).
    out may be bf16 (the logit tables of MMA(..., logit_dtype=torch.bfloat16)): the form is the one nn_form picks for an fp32 out of the
    same shape; on f16x2_k / f16x2_k256 / f16x2_k256p the kernel rounds and writes bf16 from its epilogue (BF16_EPILOGUE), on every
    other form the product goes to an fp32 temporary and rows_to_bf16 converts it - the same bits either way."""
    return _nn(a, w, out, box=row_max_box)


def rows_mm_add_(acc, a, w, row_max=None):
    """acc += a @ w in place (no autograd): the split-precision kernels fold the addition into their epilogue.  On a three-product one
    when the rows' maxima are known (row_max (M,) >= max |a[i,:]|, as K2a / K2b leave them) and the shape is the dL/dx one."""
    return _nn(a, w, acc, accumulate=True, row_max=row_max)


class _MM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _nn(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _nn(g, w.t())
        if ctx.needs_input_grad[1]:
            gw = xt_g(x, g)
        return gx, gw


def _run_tn(form, x, g, x_row_max=None, g_row_max=None):
    """x^T @ g (in,out) for tall fp32 x (N,in), g (N,out) on mma_gemm_bf16x3_tn or mma_gemm_f16x2_tn (row-strided operands are fine).
    The three-product kernel derives row scales balanced between the operands on the device from the row maxima ((N,) upper bounds of
    max |x[i,:]| / max |g[i,:]|; None = one extra pass over that operand); rows too far apart in size send it to the six-product kernel."""
    (N, KA), NC = x.shape, g.shape[1]
    f16 = form == "f16x2_tn"
    out = torch.empty((KA, NC), device=x.device, dtype=torch.float32)
    kb = _tn_cols(form, KA)
    n_ws = _lib.query("mma_gemm_%s_workspace_floats" % form, N, kb, NC)
    ws = torch.empty((n_ws,), device=x.device, dtype=torch.float32) if n_ws else None
    with _gemm_span("gemm_x3_tn", "f16x3" if f16 else "bf16x6", N, KA, NC):
        for j in range(0, KA, kb):       # one launch per column block of x (= row block of the result); the maxima of the whole row bound every block's
            # (the last block may be narrower - KA = 200 is 128 + 72: its launch is told so, it must not write kb rows into the 72 `out` has left)
            call("mma_gemm_" + form, ptr(x[:, j:j + kb]), x.stride(0), ptr(g), g.stride(0), *((ptr(x_row_max), ptr(g_row_max)) if f16 else ()),
                 ptr(out[j:j + kb]), ptr(ws), n_ws, N, min(kb, KA - j), NC, stream_ptr())
    return out


def _lib_xt_g(x, g, x_row_max=None, g_row_max=None):
    """Split-N batched library GEMM + sum (the module docstring)."""
    N = x.shape[0]
    B = N // _ROWS_PER_BATCH
    if B < 4:
        return torch.mm(x.t(), g)
    n = B * _ROWS_PER_BATCH
    x = x if x.stride(1) == 1 else x.contiguous()            # row-strided operands (column blocks of a wider buffer) are
    g = g if g.stride(1) == 1 else g.contiguous()            # fine: the row blocks stay strided-batched GEMM operands
    out = torch.bmm(x[:n].unflatten(0, (B, _ROWS_PER_BATCH)).transpose(1, 2), g[:n].unflatten(0, (B, _ROWS_PER_BATCH))).sum(0)
    if n < N:
        out = out + torch.mm(x[n:].t(), g[n:])
    return out


gemm_f16x2_tn = partial(_run_tn, "f16x2_tn")                    # (x, g, x_row_max=None, g_row_max=None)
gemm_bf16x3_tn = partial(_run_tn, "bf16x3_tn")                  # (x, g)
_TN_RUN = {"f16x2_tn": gemm_f16x2_tn, "bf16x3_tn": gemm_bf16x3_tn, "lib": _lib_xt_g}


def xt_g(x, g, x_row_max=None, g_row_max=None, named=False):
    """x^T @ g for tall x (N,in), g (N,out): the TN kernels where tn_form allows (named: as in nn_form), else the library."""
    form = "lib" if not (named or _gpu_f32(x, g, unit_cols=True)) else tn_form(
        x.shape[0], x.shape[1], g.shape[1], ldx=x.stride(0), ldg=g.stride(0), g_row_max_known=g_row_max is not None, named=named)
    return _TN_RUN[form](x, g, x_row_max, g_row_max)


def xt_g_batched(x, ka, g, nc, B):
    """(B, ka, nc): out[b] = x[:, b*ka:(b+1)*ka]^T @ g[:, b*nc:(b+1)*nc] - B independent TN products over the same rows in ONE launch
    (mma_gemm_bf16x3_tn_batched) where the shape allows, else one xt_g per block."""
    M = x.shape[0]
    if not (_gpu_f32(x, g, unit_cols=True) and tn_form(M, ka, nc, ldx=x.stride(0), ldg=g.stride(0), batch=B) == "bf16x3_tn_batched"):
        return torch.stack([xt_g(x[:, b * ka:(b + 1) * ka], g[:, b * nc:(b + 1) * nc]) for b in range(B)])
    out = torch.empty((B, ka, nc), device=x.device, dtype=torch.float32)
    n_ws = _lib.query("mma_gemm_bf16x3_tn_batched_workspace_floats", M, ka, nc, B)
    ws = torch.empty((n_ws,), device=x.device, dtype=torch.float32) if n_ws else None
    with _gemm_span("gemm_x3_tn", "bf16x6", M * B, ka, nc):
        call("mma_gemm_bf16x3_tn_batched", ptr(x), x.stride(0), ka, ptr(g), g.stride(0), nc, ptr(out), ptr(ws), n_ws, M, ka, nc, B,
             stream_ptr())
    return out


def mm(x, w):
    """x @ w with the split-reduction weight gradient."""
    return _MM.apply(x, w)


def col_sum(g):
    """g.sum(0) of a tall (R,C) fp32 matrix on the K8 kernel (fixed summation order).  torch's own column reduction
    falls off a cliff when C % 4 != 0 (3.2 ms for 204552 x 375 on MI355X; this kernel: HBM rate)."""
    _lib.require_gpu(g)
    assert g.dim() == 2 and g.dtype == torch.float32
    if g.stride(1) != 1:
        g = g.contiguous()
    R, C = g.shape
    out = torch.empty((C,), device=g.device, dtype=torch.float32)
    n_ws = int(_lib.lib().mma_col_sum_workspace_floats(R, C))
    ws = torch.empty((n_ws,), device=g.device, dtype=torch.float32) if n_ws else None
    call("mma_col_sum", ptr(g), g.stride(0) if R > 1 else C, R, C, ptr(out), ptr(ws), n_ws, stream_ptr())
    return out


_SKINNY_MIN_ROWS = 4096


def _skinny_ok(x2, weight):
    """K16: tall fp32 rows through a narrow Linear (out <= 80, in <= 512): the 75 -> 75 layers of graph regression.  rocBLAS runs
    them at ~0.11 ms per GEMM on 2e5 rows (61 MB in, 61 MB out); the fp32 matrix-core kernels stream them."""
    O, K = weight.shape
    return (x2.is_cuda and x2.dtype == torch.float32 and weight.dtype == torch.float32 and x2.dim() == 2
            and x2.shape[0] >= _SKINNY_MIN_ROWS and O <= 80 and K <= 512 and x2.stride(1) == 1
            and tower_post_fits(K, -(-O // 16)))     # the kernels' own limits (weights + wave tiles inside 160 KB of LDS, both layouts)


def tower_post_fits(KF, S):
    """mma_tower_post_fits: do K13 / K14 (K16 with S = ceil(O/16)) take a (KF, S) product?  The library answers - the gates here do
    not restate its limits (a shape inside a Python gate but outside the kernel's used to raise MMALibraryError instead of taking the
    library GEMM)."""
    return bool(_lib.query("mma_tower_post_fits", int(KF), int(S)))


def _skinny_weights(weight):
    """(Wa (KFp, S*16), Wb (S*16, KFp+16)) zero-padded copies of W (O, K) in the layouts the kernels stage into LDS."""
    O, K = weight.shape
    S = -(-O // 16)
    kfp = int(_lib.lib().mma_tower_post_kfp(K))
    Wb = torch.empty((S * 16, kfp + 16), device=weight.device, dtype=torch.float32)
    Wa = torch.empty((kfp, S * 16), device=weight.device, dtype=torch.float32)
    call("mma_skinny_linear_weights", ptr(weight.contiguous()), O, K, ptr(Wa), ptr(Wb), stream_ptr())      # one launch (a fill + two copies before)
    return Wa, Wb


SKINNY_GW = flag("MMA_SKINNY_GW")      # 0: round 4's TN GEMM + column sum (A/B)


def skinny_gw(g2, x2, want_bias=True):
    """(gw (O, K), gb (O) or None) = (g2^T x2, column sums of g2) for tall fp32 rows, O <= 80, K <= 512: mma_skinny_linear_gw."""
    rows, O = g2.shape
    K = x2.shape[1]
    n_part = int(_lib.query("mma_skinny_linear_gw_part", rows, K, O))
    part = torch.empty(n_part, device=g2.device, dtype=torch.float32)
    gw = torch.empty((O, K), device=g2.device, dtype=torch.float32)
    gb = torch.empty(O, device=g2.device, dtype=torch.float32) if want_bias else None
    with _span("skinny_linear_gw", nbytes=4 * rows * (K + O), flops=2 * rows * (-(-O // 16) * 16) * (-(-(K + 1) // 16) * 16), mfma="f32"):
        call("mma_skinny_linear_gw", ptr(g2), g2.stride(0), ptr(x2), x2.stride(0), ptr(part), n_part, ptr(gw), ptr(gb), rows, K, O, stream_ptr())
    return gw, gb


class _Linear(torch.autograd.Function):
    """y = x W^T + b over the last dimension (torch_geometric Linear / F.linear: mma_conv.py:82,99-105, mask_aggr.py:50).
    Forward is the library GEMM - or, for tall rows through a narrow layer, the K16 fp32 matrix-core kernel; backward replaces
    autograd's weak spots for tall inputs: the weight gradient is the split-reduction GEMM (xt_g), the bias gradient the K8 column
    sum, dL/dx the K16 kernel again."""

    @staticmethod
    def forward(ctx, x, weight, bias, addend=None):
        """addend (rows, out), optional: y = linear(x) + addend - on the K16 path the addition is the kernel's epilogue (one pass less over
        two (rows, out) tensors and one launch less: MMAConv's post-NN, y_aggregates + x W_x^T + b)."""
        ctx.has_bias = bias is not None
        x2 = x.reshape(-1, x.shape[-1])
        ctx.skinny = _skinny_ok(x2, weight)
        if ctx.skinny:
            O, K = weight.shape
            Wa, Wb = _skinny_weights(weight)
            y = torch.empty((x2.shape[0], O), device=x.device, dtype=torch.float32)
            add2 = None
            if addend is not None:
                add2 = addend.reshape(-1, O)
                add2 = add2 if add2.stride(1) == 1 else add2.contiguous()
            x3 = add2 is None and flag("MMA_SKINNY_X3") and not flag("MMA_POST_EXACT", default=False)
            with _span("skinny_linear_fwd", nbytes=4 * x2.shape[0] * (K + O * (2 if add2 is not None else 1)), flops=2 * x2.shape[0] * Wa.shape[0] * Wa.shape[1],
                       mfma="bf16x6" if x3 else "f32"):
                call("mma_skinny_linear_fwd", ptr(x2), x2.stride(0), ptr(Wa), ptr(bias.contiguous() if bias is not None else None), ptr(add2),
                     add2.stride(0) if add2 is not None else 0, ptr(y), O, x2.shape[0], K, O, stream_ptr())
            ctx.save_for_backward(x, weight, Wb)
            return y.view(x.shape[:-1] + (O,))
        ctx.save_for_backward(x, weight)
        y = torch.nn.functional.linear(x, weight, bias)
        return y if addend is None else y + addend.reshape(y.shape)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors[:2]
        g2 = g.reshape(-1, g.shape[-1])
        gx = gw = gb = None
        g_add = g if (len(ctx.needs_input_grad) > 3 and ctx.needs_input_grad[3]) else None      # d(y)/d(addend) = identity
        if ctx.needs_input_grad[0]:
            if ctx.skinny:
                O, K = weight.shape
                g2 = g2 if g2.stride(1) == 1 else g2.contiguous()
                gx2 = torch.empty((g2.shape[0], K), device=g.device, dtype=torch.float32)
                Wb_ = ctx.saved_tensors[2]
                with _span("skinny_linear_bwd", nbytes=4 * g2.shape[0] * (K + O), flops=2 * g2.shape[0] * Wb_.shape[0] * (Wb_.shape[1] - 16), mfma="f32"):
                    call("mma_skinny_linear_bwd_dx", ptr(g2), g2.stride(0), ptr(ctx.saved_tensors[2]), ptr(gx2), K, g2.shape[0], K, O, stream_ptr())
                gx = gx2.view(x.shape)
            else:
                gx = torch.mm(g2, weight).view(x.shape)
        x2 = x.reshape(-1, x.shape[-1])
        if ctx.skinny and SKINNY_GW and ctx.needs_input_grad[1] and x2.stride(1) == 1:
            # K15 in its plain form: the weight and the bias gradient from ONE pass over g and x (the bias gradient as the product with a
            # ones column behind x) - the TN library GEMM + the column sum read g twice and took ~0.09 ms per 75 -> 75 layer at C2L
            gw, gb = skinny_gw(g2 if g2.stride(1) == 1 else g2.contiguous(), x2, ctx.has_bias and ctx.needs_input_grad[2])
            return gx, gw, gb, g_add
        if ctx.has_bias and ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and x2.shape[0] >= 4 * _ROWS_PER_BATCH and not ctx.skinny:
            # tall input: the bias gradient rides on the weight-gradient GEMM as the row of a ones column appended to x, so the
            # (rows, out) gradient is read once instead of twice (C2L: 2 x 0.13 ms of column sums over 0.62 / 0.65 GB)
            gw1 = xt_g(g2, torch.cat([x2, x2.new_ones((x2.shape[0], 1))], 1))               # (out, in + 1)
            return gx, gw1[:, :-1].contiguous(), gw1[:, -1].contiguous(), g_add
        if ctx.needs_input_grad[1]:
            gw = xt_g(g2, x2)                                           # (out, in)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = col_sum(g2)
        return gx, gw, gb, g_add


def linear(x, weight, bias=None, addend=None):
    """F.linear (+ addend) with the tall-input backward (GPU tensors only)."""
    return _Linear.apply(x, weight, bias, addend)


# ---- tall Linear layers with odd widths on the bf16x3 kernels (graph regression: 75 -> 760 on 2e5 rows, 50 -> 380 on 4e5) ------
# rocBLAS runs these at 30-60 TFLOP/s (K or N in {50, 75, 76, 380, 760}: nothing is a multiple of anything); zero-padded to
# K = 128 and N % 128 == 0 they are ordinary inputs of the bf16x3 kernels.  The ones column that carries the bias sits in the
# K padding, so forward folds the bias in and the TN weight-gradient GEMM returns the bias gradient as one more row.
X3_LINEAR = True
FUSED_PAD = flag("MMA_PAD_ONES")        # 0: torch's pad + a strided fill (round 3)
X3_LINEAR_MIN_ROWS = 32768
_PADDED = {}          # data_ptr -> weakref to a (rows, pitch) fp32 buffer whose columns beyond the payload are ZERO


def _round_up(v, m):
    return -(-v // m) * m


def padded_empty(rows, cols, device, multiple=128, row_max=None):
    """The (rows, cols) leading-columns view of a new (rows, round_up(cols, multiple)) fp32 buffer whose pad columns are zero
    and which is REGISTERED: a consumer (linear_x3's backward) can take the whole buffer as a GEMM operand without a copy.
    Producers that fill such a view must leave the pad columns alone.  row_max (rows,), optional: the producer will leave
    max |row| there (K4 / the dV segment sum, round 5) - it travels with the buffer, and the consumer's GEMMs take the three-product form."""
    import weakref
    pitch = _round_up(cols, multiple)
    buf = torch.empty((rows, pitch), device=device, dtype=torch.float32)
    buf._mma_row_max = row_max
    if pitch > cols:
        buf[:, cols:].zero_()
    for k in [k for k, r in _PADDED.items() if r() is None]:
        del _PADDED[k]
    _PADDED[buf.data_ptr()] = weakref.ref(buf)
    return buf[:, :cols]


def _padded_parent(v, pitch):
    ref = _PADDED.get(v.data_ptr())
    buf = ref() if ref is not None else None
    if (buf is not None and v.dim() == 2 and tuple(buf.shape) == (v.shape[0], pitch) and v.stride(1) == 1 and v.stride(0) == pitch
            and v.storage_offset() == buf.storage_offset() and v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()):
        return buf
    return None


class _LinearX3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, row_index=None, inv_index=None):
        """row_index (N,) int32 / inv_index (N,) int64, a permutation and its inverse (optional): y = linear(x[row_index]) - the gather rides
        on the pad launch (graph regression's edge rows in target-sorted position order), dL/dx is gathered back with inv_index."""
        N, fin = x.shape
        ctx.inv_index = inv_index
        fout = weight.shape[0]
        OP = _round_up(fout, 128)
        fused = FUSED_PAD and _gpu_f32(x, unit_cols=True) and weight.dtype == torch.float32
        # [r5] the A operand is padded to 64 / 96 columns where [x | 1] fits (edge features 50 + 1, node features 75 + 1): the forward and
        # the weight-gradient product stop reading, splitting and multiplying pad columns up to 128 - where the forward product runs on the
        # whole-row kernel: the general kernel behind it takes K % 128 == 0 only
        KP = next(k for k in F16X2_K if fin + 1 <= k)
        KP = KP if nn_form(N, KP, OP, named=True) == "f16x2_k" else 128
        if row_index is not None and not fused:
            x = x.index_select(0, row_index.long())
        if fused:
            # [r4] both padded operands in ONE launch each (mma_pad_rows): A = [x | 1 | 0] (N, 128), and wpad = [W | b | 0] (OP, 128), whose
            # transposed VIEW is the forward's B and whose leading columns are dL/dx's B - no second padded copy of W in backward
            xp = torch.empty((N, KP), device=x.device, dtype=torch.float32)
            call("mma_pad_rows", ptr(x), x.stride(0), N, fin, None, ptr(row_index), ptr(xp), KP, KP, N, stream_ptr())
            w2 = weight if weight.stride(1) == 1 else weight.contiguous()
            wpad = torch.empty((OP, 128), device=x.device, dtype=torch.float32)
            if bias is not None:
                call("mma_pad_rows", ptr(w2), w2.stride(0), fout, fin, ptr(bias.contiguous()), None, ptr(wpad), 128, 128, OP, stream_ptr())
            else:
                call("mma_pad_rows", ptr(w2), w2.stride(0), fout, fin + 0, ptr(torch.zeros((fout,), device=x.device)), None, ptr(wpad), 128, 128, OP, stream_ptr())
            wt = wpad.t()[:KP]                                       # (KP, OP) view: rows beyond fin + 1 are zero anyway
        else:
            xp = torch.nn.functional.pad(x, (0, KP - fin))          # (N, KP): [x | 1 | 0 ...]
            xp[:, fin] = 1.0
            wt = weight.new_zeros((KP, OP))                          # [W^T ; b ; 0 ...], pad columns zero
            wt[:fin, :fout] = weight.t()
            if bias is not None:
                wt[fin, :fout] = bias
            wpad = None
        box = []
        y = gemm_bf16x3(xp, wt, row_max_box=box)                     # (N, OP); columns beyond fout are exact zeros
        ctx.x_rm = box[0] if box else None                           # max |[x | 1]| per row, formed by the three-product forward for its own scales
        if wpad is not None:
            ctx.save_for_backward(xp, weight, wpad)
        else:
            ctx.save_for_backward(xp, weight)
        ctx.dims = (fin, fout, OP, bias is not None)
        return y[:, :fout]

    @staticmethod
    def backward(ctx, g):
        xp, weight = ctx.saved_tensors[:2]
        wpad = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        fin, fout, OP, has_bias = ctx.dims
        gp = _padded_parent(g, OP)                                   # the producer's own zero-padded buffer: no copy
        if gp is None:
            gp = torch.nn.functional.pad(g, (0, OP - fout))
        gx = gw = gb = None
        # [r5] the producer of g (K4 + the dV segment sum) left max |g row| with its padded buffer: both products take the THREE-product
        # fp16 x 2 kernels (round 4: six bf16 products, because nobody knew the row maxima - 15 % of the C2L step)
        g_rm = getattr(gp, "_mma_row_max", None)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gwb = xt_g(xp[:, :_round_up(fin + 1, 32)], gp, ctx.x_rm, g_rm, named=True)                 # (KA, OP) = [x | 1]^T g
            gw = gwb[:fin, :fout].t().contiguous()
            gb = gwb[fin, :fout].contiguous() if has_bias else None
        if ctx.needs_input_grad[0] and g_rm is not None and wpad is not None and f16x2_n128_ok(gp.shape[0], OP, 128):
            # dL/dx = g [W | b | 0]: one pass over g on the one-accumulator kernel; column `fin` (the bias column) is dropped by the slice
            gx = gemm_f16x2_n128(gp, g_rm, wpad, torch.empty((gp.shape[0], 128), device=gp.device, dtype=torch.float32))[:, :fin]
        elif ctx.needs_input_grad[0]:
            NP = _round_up(fin, 32)
            if wpad is not None:
                wp = wpad[:, :NP]           # column fin (the bias) lands in a pad column of gx that the slice below drops
            else:
                wp = weight.new_zeros((OP, NP))
                wp[:fout, :fin] = weight
            gx = gemm_bf16x3(gp, wp)[:, :fin]
        if gx is not None and ctx.inv_index is not None:
            gx = gx.index_select(0, ctx.inv_index)                   # back to the caller's row order (deterministic: a gather, no index_add)
        return gx, gw, gb, None, None


def linear_x3_ok(x, weight):
    return (X3_LINEAR and x.dim() == 2 and _gpu_f32(x) and x.shape[0] >= X3_LINEAR_MIN_ROWS
            and x.shape[1] + 1 <= 128 and weight.shape[0] > 128)      # narrower outputs: measured no better than the library (A is split per 4 tiles only)


def linear_tall(x, weight, bias=None):
    """F.linear for a tall 2-D x: zero-padded onto the bf16x3 kernels where that pays (see above), else `linear`."""
    if linear_x3_ok(x, weight):
        return _LinearX3.apply(x, weight, bias, None, None)
    return _Linear.apply(x, weight, bias, None)


def linear_tall_rows(x, row_index, inv_index, weight, bias=None):
    """linear_tall(x[row_index]) for a PERMUTATION row_index (int32) with inverse inv_index (int64): on the zero-padded path the gather
    is part of the pad launch; None: the caller permutes first."""
    if linear_x3_ok(x, weight) and FUSED_PAD and x.stride(1) == 1:
        return _LinearX3.apply(x, weight, bias, row_index, inv_index)
    return None


class _BiasAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, b):
        return y + b

    @staticmethod
    def backward(ctx, g):
        return g, (col_sum(g.reshape(-1, g.shape[-1])) if ctx.needs_input_grad[1] else None)


def bias_add(y, b):
    """y (..., C) + b (C,) whose bias gradient is the K8 column sum."""
    return _BiasAdd.apply(y, b)


class _TowerLinear(torch.autograd.Function):
    """y[n,t,:] = a[n,t,:] @ W[t]^T for a (N,T,C), W (T,O,C): the per-tower post-NN Linear of MMAConv (mma_conv.py:132-134)
    on the aggregates, without slicing towers apart.  Backward writes the gradient of `a` tower by tower straight into
    its (N,T,C) layout (autograd's batched GEMM returns it tower-major and costs a 1.9 GB re-layout copy at C2L) and takes
    the weight gradients as split-reduction GEMMs over the row-strided tower slices."""

    @staticmethod
    def forward(ctx, a, W):
        ctx.save_for_backward(a, W)
        return torch.bmm(a.transpose(0, 1), W.transpose(1, 2)).transpose(0, 1)

    @staticmethod
    def backward(ctx, g):
        a, W = ctx.saved_tensors
        T, O, C = W.shape
        N = a.shape[0]
        if (a.is_cuda and O <= 16 and C % 4 == 0 and N > 0 and a.is_contiguous() and ctx.needs_input_grad[0]
                and ctx.needs_input_grad[1]):
            # K9: both gradients in one pass over `a` (the 15-wide batched GEMMs below run at ~15 TFLOP/s)
            g = g.contiguous()
            Wc = W.contiguous()
            ga = torch.empty_like(a)
            nb = int(_lib.lib().mma_tower_linear_bwd_blocks(N))
            part = torch.empty((nb, T * O * C), device=a.device, dtype=torch.float32)
            call("mma_tower_linear_bwd", ptr(g), ptr(a), ptr(Wc), ptr(ga), ptr(part), nb, N, T, O, C, stream_ptr())
            return ga, col_sum(part).view(T, O, C)
        ga = gW = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(a, memory_format=torch.contiguous_format)
            torch.bmm(g.transpose(0, 1), W, out=ga.transpose(0, 1))          # strided-batched: ldc = T*C, batch stride C
        if ctx.needs_input_grad[1]:
            gW = torch.stack([xt_g(g[:, t], a[:, t]) for t in range(T)])
        return ga, gW


def tower_linear(a, W):
    return _TowerLinear.apply(a, W)
