"""4-bit block-quantised Llama projections for the evaluation path (include/vaa_model_ops.h states the format; csrc/vaa_quant.hip holds the
two kernels): what the reference's evaluation gets from `from_pretrained(..., load_in_4bit=True)` (experiments/robot/openvla_utils.py:43-51),
built here because bitsandbytes does not exist on this platform. Inference only: `predict_action` and `evaluate_patch` run on a quantised
model, the training entry points refuse it.

  quantize_q4 / dequantize_q4   the quantiser and its inverse in torch (CPU and GPU give the same codes: every comparison is exact)
  q4_linear                     vaa_model_q4_gemv for at most GEMV_MAX_ROWS rows of a decode step, vaa_model_q4_dequant into one shared scratch +
                                the stock GEMM otherwise and always in prefill
  Q4Linear / Q4LinearRows       codes + absmax as buffers, the table, no `weight`; the rows of a fused parent as a module of their own
Neither table could be compared with bitsandbytes in this image; the fp4 entries are stated from memory.

The 8-bit format (`load_in_8bit` in the reference: LLM.int8) lives here as well — csrc/vaa_quant8.hip, stated in the same header, likewise not
compared with bitsandbytes:
  quantize_q8 / dequantize_q8   int8 codes with one fp32 scale per row, and the dequantised weight
  q8_linear                     vaa_model_q8_act_quant + vaa_model_q8_matmul on a GPU, q8_linear_torch (the same arithmetic in torch) elsewhere
  Q8Linear / Q8LinearRows       codes + wscale as buffers and the outlier threshold of the layer's calls

Both formats share one host shape (QuantLinear, the row views of a fused parent) and one place in the model:
  quantize_llm                  the seven projections of every LlamaLayer -> Q4Linear or Q8Linear ("int8"); towers, projector, embeddings and
                                lm_head stay bf16. Sets `quant_type` on the model and its layers and installs QuantProjections on each layer
  QuantProjections              the quantised kinds of the projections in LlamaLayer.prefill / decode_step. The inference graph is stated there,
                                once, for bf16, 4-bit and int8 weights; a kind only says how a projection is formed
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

BLOCK = 64
GEMV_MAX_ROWS = 16  # vaa_model_q4_gemv's limit on M; more rows take dequant + GEMM

_NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
        -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
        0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)  # QLoRA (Dettmers et al. 2023), appendix E
_FP4_MAG = (0.0, 1.0 / 192.0, 2.0 / 3.0, 1.0, 1.0 / 3.0, 0.5, 1.0 / 6.0, 0.25)  # bitsandbytes' sign-magnitude table: bits 0-2, bit 3 = sign


def _f32(v) -> float:
    return ctypes.c_float(float(v)).value


TABLES = {
    "nf4": tuple(_f32(v) for v in _NF4),
    "fp4": tuple(_f32(v) for v in _FP4_MAG) + tuple(_f32(-v) for v in _FP4_MAG),
}


def table_values(table) -> tuple:
    """A table name ("nf4", "fp4") or 16 values -> the 16 values as Python floats that are exact fp32 numbers."""
    if isinstance(table, str):
        if table not in TABLES:
            raise ValueError(f"unknown 4-bit table {table!r} (known: {sorted(TABLES)})")
        return TABLES[table]
    vals = tuple(_f32(v) for v in (table.tolist() if isinstance(table, torch.Tensor) else table))
    if len(vals) != 16 or any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        raise ValueError("a 4-bit table is 16 finite values")
    return vals


def _sorted_table(tab, device):
    """(mids float64 [U-1], index int64 [U]): the distinct table values in ascending order (for equal values, -0.0 and 0.0 among them, the
    SMALLEST table index stands), and the exact midpoints of neighbours (the sum of two fp32 numbers is exact in fp64)."""
    first = {}
    for i, v in enumerate(tab):
        first.setdefault(v + 0.0, i)  # -0.0 == 0.0 as a key
    vals = sorted(first)
    mids = [(a + b) / 2.0 for a, b in zip(vals[:-1], vals[1:])]
    return torch.tensor(mids, dtype=torch.float64, device=device), torch.tensor([first[v] for v in vals], dtype=torch.int64, device=device)


@torch.no_grad()
def quantize_q4(w: torch.Tensor, table, rows_per_pass: int = 1024):
    """W [N,K] (bf16 or fp32; K % 64 == 0) -> (codes uint8 [N,K/2], absmax float32 [N,K/64]) in the format of include/vaa_model_ops.h, on W's
    device. Exact on every device: the fp32 quotient is the fp64 quotient rounded to fp32 (53 >= 2*24 + 2 bits: the correctly rounded fp32
    division), and the nearest entry is found by comparing it, in fp64, with the exact midpoints of the sorted table — on a midpoint, and
    between equal entries, the smaller table index wins; a block whose absmax is 0 maps to the quotient 0, i.e. to the table's first 0."""
    tab = table_values(table)
    if w.dim() != 2 or w.shape[1] % BLOCK != 0 or w.shape[1] < BLOCK:
        raise ValueError(f"quantize_q4: W must be [N,K] with K a positive multiple of {BLOCK}, got {tuple(w.shape)}")
    N, K = w.shape
    mids, index = _sorted_table(tab, w.device)
    codes = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    absmax = torch.empty((N, K // BLOCK), dtype=torch.float32, device=w.device)
    for r0 in range(0, N, rows_per_pass):
        wf = w[r0:r0 + rows_per_pass].to(torch.float32).reshape(-1, K // BLOCK, BLOCK)
        am = wf.abs().amax(-1)
        absmax[r0:r0 + rows_per_pass] = am
        amd = am.to(torch.float64)[..., None]
        quot = torch.where(amd > 0, wf.to(torch.float64) / amd, torch.zeros((), dtype=torch.float64, device=w.device))
        quot = quot.to(torch.float32).to(torch.float64)
        j = torch.bucketize(quot, mids)  # mids[j-1] < quot <= mids[j]: a quotient ON a midpoint lands on the lower neighbour
        if mids.numel():
            jn = j.clamp_max(mids.numel() - 1)
            tie = (j < mids.numel()) & (quot == mids[jn])
            q = torch.where(tie, torch.minimum(index[jn], index[jn + 1]), index[j])
        else:
            q = index[j]
        q = q.reshape(-1, K).to(torch.uint8)
        codes[r0:r0 + rows_per_pass] = (q[:, 0::2] << 4) | q[:, 1::2]
    return codes, absmax


@torch.no_grad()
def dequantize_q4(codes: torch.Tensor, absmax: torch.Tensor, table) -> torch.Tensor:
    """(codes [N,K/2], absmax [N,K/64]) -> the dequantised weight bf16 [N,K] = bf16(table[q] * absmax): one fp32 product, one rounding."""
    tab = torch.tensor(table_values(table), dtype=torch.float32, device=codes.device)
    N, K = codes.shape[0], codes.shape[1] * 2
    q = torch.stack([codes >> 4, codes & 15], dim=-1).reshape(N, K).to(torch.int64)
    return (tab[q].reshape(N, K // BLOCK, BLOCK) * absmax[..., None]).reshape(N, K).to(torch.bfloat16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class QuantLinear(nn.Module):
    """What Q4Linear and Q8Linear share: a frozen bias-free linear layer held as a buffer `codes` [out, ...] and its scales, without a
    `weight` (`dequantize()` forms it), called through its format's product on 2-D rows (`linear2d`: q4_linear / q8_linear)."""

    @property
    def out_features(self) -> int:
        return int(self.codes.shape[0])

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, quant_type={self.quant_type}"

    @torch.no_grad()
    def forward(self, x, res=None, scratch=None, gemv=True):
        """linear2d on the last axis of x (inference only): ALL leading axes form the rows of one call."""
        y = self.linear2d(x.reshape(-1, x.shape[-1]), None if res is None else res.reshape(-1, self.out_features), scratch, gemv)
        return y.view(*x.shape[:-1], self.out_features)


class _FusedRows:
    """Rows [row0, row0 + rows) of a fused QuantLinear (q / k / v of the row-concatenated qkv codes, gate / up likewise): the projection as a
    module of its own without a second copy of its codes. A subclass names the parent's buffers that it slices and the settings it takes over."""

    def __init_subclass__(cls, buffers=(), settings=(), **kw):
        super().__init_subclass__(**kw)
        cls._settings = settings
        for name in buffers:
            setattr(cls, name, property(lambda self, name=name: getattr(self._src[0], name)[self.row0:self.row0 + self.rows]))

    def __init__(self, parent: QuantLinear, row0: int, rows: int):
        nn.Module.__init__(self)
        for name in self._settings:
            setattr(self, name, getattr(parent, name))
        self._src = (parent,)  # in a tuple: the parent is registered once, on the layer
        self.row0, self.rows = int(row0), int(rows)


def q4_dequant(codes: torch.Tensor, absmax: torch.Tensor, table, out: torch.Tensor | None = None) -> torch.Tensor:
    """The dequantised weight [N,K] bf16 through vaa_model_q4_dequant on a GPU (into `out`, a contiguous buffer of at least N*K bf16, when
    given), through dequantize_q4 elsewhere."""
    N, K = codes.shape[0], codes.shape[1] * 2
    if not codes.is_cuda:
        w = dequantize_q4(codes, absmax, table)
        return w if out is None else out.reshape(-1)[:N * K].view(N, K).copy_(w)
    if not (codes.is_contiguous() and absmax.is_contiguous()):
        raise ValueError("q4_dequant: codes and absmax must be contiguous")
    w = torch.empty((N, K), dtype=torch.bfloat16, device=codes.device) if out is None else out.reshape(-1)[:N * K].view(N, K)
    rc = _lib.lib().vaa_model_q4_dequant(codes.data_ptr(), absmax.data_ptr(), _lib.f32x(table_values(table)), N, K, w.data_ptr(), _stream())
    _lib.check(rc, "vaa_model_q4_dequant")
    return w


def q4_gemv(x: torch.Tensor, codes: torch.Tensor, absmax: torch.Tensor, table, res: torch.Tensor | None = None) -> torch.Tensor:
    """bf16(res + x @ wq^T) for x bf16 [M,K], 1 <= M <= 16, through vaa_model_q4_gemv (a GPU is required: no other formulation hides here)."""
    M, K = x.shape
    N = codes.shape[0]
    if codes.shape[1] * 2 != K or x.dtype != torch.bfloat16 or not (x.is_contiguous() and codes.is_contiguous() and absmax.is_contiguous()):
        raise ValueError("q4_gemv: x must be contiguous bf16 [M,K] and codes / absmax contiguous [N,K/2] / [N,K/64]")
    if res is not None and (res.shape != (M, N) or res.dtype != torch.bfloat16 or not res.is_contiguous()):
        raise ValueError("q4_gemv: res must be contiguous bf16 [M,N]")
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    rc = _lib.lib().vaa_model_q4_gemv(x.data_ptr(), M, codes.data_ptr(), absmax.data_ptr(), _lib.f32x(table_values(table)), N, K,
                                      res.data_ptr() if res is not None else None, y.data_ptr(), _stream())
    _lib.check(rc, "vaa_model_q4_gemv")
    return y


class Q4Linear(QuantLinear):
    """A frozen bias-free linear layer held as 4-bit codes: buffers `codes` uint8 [out,in/2] and `absmax` float32 [out,in/64], the table's
    name and values. There is no `weight`; `dequantize()` forms it."""

    def __init__(self, codes: torch.Tensor, absmax: torch.Tensor, quant_type):
        super().__init__()
        self.quant_type = quant_type if isinstance(quant_type, str) else "custom"
        self.table = table_values(quant_type)
        self.register_buffer("codes", codes)
        self.register_buffer("absmax", absmax)

    @classmethod
    def from_weight(cls, w: torch.Tensor, quant_type) -> "Q4Linear":
        return cls(*quantize_q4(w, quant_type), quant_type)

    @property
    def in_features(self) -> int:
        return int(self.codes.shape[1]) * 2

    def dequantize(self) -> torch.Tensor:
        return dequantize_q4(self.codes, self.absmax, self.table)

    def linear2d(self, x2, res=None, scratch=None, gemv=True):
        """bf16(res + x2 @ wq^T): q4_linear."""
        return q4_linear(x2, self, res, scratch, gemv)


class Q4LinearRows(_FusedRows, Q4Linear, buffers=("codes", "absmax"), settings=("quant_type", "table")):
    """Rows of a fused Q4Linear. Blocks never cross a row, so the slice is exactly the projection's own codes."""


class Q4Scratch:
    """One bf16 buffer of the largest single projection (llm_mlp x llm_dim), shared by every layer of a quantised model: the target of
    vaa_model_q4_dequant on the dequant + GEMM route. Allocated on first use, per device."""

    def __init__(self, elems: int):
        self.elems = int(elems)
        self._buf = None

    def get(self, device) -> torch.Tensor:
        if self._buf is None or self._buf.device != device:
            self._buf = torch.empty(self.elems, dtype=torch.bfloat16, device=device)
        return self._buf


def q4_linear(x2: torch.Tensor, lin: Q4Linear, res: torch.Tensor | None = None, scratch: Q4Scratch | None = None, gemv: bool = True) -> torch.Tensor:
    """bf16(res + x2 @ wq^T) for x2 [M,K]. bf16 on a GPU: vaa_model_q4_gemv when `gemv` and M <= GEMV_MAX_ROWS, else vaa_model_q4_dequant into
    the scratch (in row ranges that fit it) + the stock GEMM with the residual in its epilogue. Elsewhere (CPU plumbing tests): dequantize_q4 +
    the stock GEMM."""
    M, K = x2.shape
    N = lin.out_features
    codes, absmax = lin.codes, lin.absmax
    if x2.is_cuda and x2.dtype == torch.bfloat16:
        if gemv and 1 <= M <= GEMV_MAX_ROWS:
            return q4_gemv(x2.contiguous(), codes, absmax, lin.table, None if res is None else res.contiguous())
        buf = scratch.get(x2.device) if scratch is not None else torch.empty(N * K, dtype=torch.bfloat16, device=x2.device)
        step = buf.numel() // K
        step = step // 4 * 4 if step >= 4 else max(1, step)  # a row range's absmax starts 16-byte aligned even at K = 64
        out = None if step >= N else torch.empty((M, N), dtype=torch.bfloat16, device=x2.device)
        for a in range(0, N, step):
            b = min(N, a + step)
            w = q4_dequant(codes[a:b], absmax[a:b], lin.table, out=buf)
            y = F.linear(x2, w) if res is None else torch.addmm(res[:, a:b], x2, w.t())
            if out is None:
                return y
            out[:, a:b] = y
        return out
    w = dequantize_q4(codes, absmax, lin.table).to(x2.dtype)
    return F.linear(x2, w) if res is None else torch.addmm(res, x2, w.t())


# ---- the 8-bit format (include/vaa_model_ops.h, "8-bit weights and activations with bf16 outlier columns"; csrc/vaa_quant8.hip) ----
INT8 = "int8"
Q8_MAX_K = 133120        # 127^2 K < 2^31
Q8_GEMV_MAX_ROWS = 16    # vaa_model_q8_matmul: at most this many rows take the split-K form, more the tiled integer GEMM
Q8_TORCH_ROUTE = False   # tests: run q8_linear's torch formulation on the GPU as well


def _div32(a: torch.Tensor, b) -> torch.Tensor:
    """The correctly rounded fp32 quotient on every device: the fp64 quotient rounded to fp32 (53 >= 2*24 + 2 bits)."""
    b = b.to(torch.float64) if isinstance(b, torch.Tensor) else float(b)
    return (a.to(torch.float64) / b).to(torch.float32)


@torch.no_grad()
def quantize_q8(w: torch.Tensor, rows_per_pass: int = 1024):
    """W [N,K] (bf16 or fp32 holding bf16 values; K % 64 == 0) -> (codes int8 [N,K], wscale float32 [N]) in the format of
    include/vaa_model_ops.h, on W's device, the same codes on every device: wscale = the row's absmax, code = rint(127 W / wscale) with the
    product exact and the quotient formed in fp64 (never within rounding distance of a tie), clamped to +-127; a zero row gives zero codes."""
    if w.dim() != 2 or w.shape[1] % 64 != 0 or not 64 <= w.shape[1] <= Q8_MAX_K:
        raise ValueError(f"quantize_q8: W must be [N,K] with K a multiple of 64 in 64 .. {Q8_MAX_K}, got {tuple(w.shape)}")
    N, K = w.shape
    codes = torch.empty((N, K), dtype=torch.int8, device=w.device)
    wscale = torch.empty((N,), dtype=torch.float32, device=w.device)
    for r0 in range(0, N, rows_per_pass):
        wf = w[r0:r0 + rows_per_pass].to(torch.float32)
        ws = wf.abs().amax(-1)
        wscale[r0:r0 + rows_per_pass] = ws
        wd = ws.to(torch.float64)[:, None]
        quot = torch.where(wd > 0, 127.0 * wf.to(torch.float64) / wd, torch.zeros((), dtype=torch.float64, device=w.device))
        codes[r0:r0 + rows_per_pass] = torch.round(quot).clamp_(-127, 127).to(torch.int8)  # torch.round: half to even
    return codes, wscale


@torch.no_grad()
def dequantize_q8(codes: torch.Tensor, wscale: torch.Tensor) -> torch.Tensor:
    """(codes int8 [N,K], wscale [N]) -> wdq bf16 [N,K] = bf16((float(q) * wscale) / 127): one fp32 product, one fp32 division, one rounding."""
    return _div32(codes.to(torch.float32) * wscale.to(torch.float32)[:, None], 127.0).to(torch.bfloat16)


@torch.no_grad()
def q8_act_quant_torch(x2: torch.Tensor, threshold: float):
    """The activation rule in torch (any device): (xq float32 [M,K] holding the integers, ascale float32 [M], outlier mask bool [K])."""
    xf = x2.to(torch.float32)
    ax = xf.abs()
    outl = ax.amax(0) >= threshold if threshold > 0 else torch.zeros(xf.shape[1], dtype=torch.bool, device=xf.device)
    ascale = ax.masked_fill(outl[None, :], 0.0).amax(1)
    inv = torch.where(ascale > 0, _div32(torch.full_like(ascale, 127.0), ascale.clamp_min(1e-45)), torch.zeros_like(ascale))
    xq = torch.round(xf * inv[:, None]).clamp_(-127, 127)
    xq = xq.masked_fill(outl[None, :] | (ascale == 0)[:, None], 0.0)
    return xq, ascale, outl


@torch.no_grad()
def q8_linear_torch(x2: torch.Tensor, codes: torch.Tensor, wscale: torch.Tensor, res: torch.Tensor | None, threshold: float) -> torch.Tensor:
    """The arithmetic of vaa_model_q8_act_quant + vaa_model_q8_matmul in torch, step by step as the header states it: the integer sum through
    an fp64 product (exact: below 2^31), every fp32 step an elementwise torch operation, the divisions through _div32."""
    xq, ascale, outl = q8_act_quant_torch(x2, threshold)
    xf = x2.to(torch.float32)
    acc = (xq.to(torch.float64) @ codes.to(torch.float64).t()).to(torch.float32)  # float(acc): round to nearest even
    y = _div32(acc * (ascale[:, None] * wscale[None, :]), 16129.0)
    o = torch.zeros_like(y)
    for k in outl.nonzero().flatten().tolist():  # ascending
        wdq = _div32(codes[:, k].to(torch.float32) * wscale, 127.0).to(torch.bfloat16).to(torch.float32)
        prod = xf[:, k:k + 1] * wdq[None, :]
        o = o + prod
    y = y + o
    if res is not None:
        y = y + res.to(torch.float32)
    return y.to(torch.bfloat16)


class Q8Scratch:
    """The per-call buffers of vaa_model_q8_act_quant (xq, ascale, the K + 1 outlier words), shared by every layer of a converted model and
    grown on demand; calls on one stream are ordered, so the next projection may overwrite them."""

    def __init__(self):
        self._xq = self._as = self._out = None

    def get(self, M: int, K: int, device):
        if self._xq is None or self._xq.device != device or self._xq.numel() < M * K:
            self._xq = torch.empty(M * K, dtype=torch.int8, device=device)
        if self._as is None or self._as.device != device or self._as.numel() < M:
            self._as = torch.empty(M, dtype=torch.float32, device=device)
        if self._out is None or self._out.device != device or self._out.numel() < K + 1:
            self._out = torch.empty(K + 1, dtype=torch.int32, device=device)
        return self._xq[:M * K].view(M, K), self._as[:M], self._out[:K + 1]


def q8_act_quant(x2: torch.Tensor, threshold: float, scratch: Q8Scratch | None = None):
    """vaa_model_q8_act_quant on contiguous bf16 x2 [M,K] (a GPU is required): (xq int8 [M,K], ascale float32 [M], outliers int32 [K+1] =
    the count, then the outlier columns in ascending order)."""
    M, K = x2.shape
    if x2.dtype != torch.bfloat16 or not x2.is_contiguous():
        raise ValueError("q8_act_quant: x must be contiguous bf16 [M,K]")
    xq, ascale, outl = (scratch or Q8Scratch()).get(M, K, x2.device)
    rc = _lib.lib().vaa_model_q8_act_quant(x2.data_ptr(), M, K, float(threshold), xq.data_ptr(), ascale.data_ptr(), outl.data_ptr(), _stream())
    _lib.check(rc, "vaa_model_q8_act_quant")
    return xq, ascale, outl


def q8_matmul(xq, ascale, outl, x2, codes, wscale, res=None) -> torch.Tensor:
    """vaa_model_q8_matmul on what q8_act_quant returned: y bf16 [M,N]; at most Q8_GEMV_MAX_ROWS rows take the split-K form."""
    M, K = x2.shape
    N = codes.shape[0]
    if codes.shape[1] != K or codes.dtype != torch.int8 or not (codes.is_contiguous() and wscale.is_contiguous()):
        raise ValueError("q8_matmul: codes / wscale must be contiguous int8 [N,K] / float32 [N]")
    if res is not None and (res.shape != (M, N) or res.dtype != torch.bfloat16 or not res.is_contiguous()):
        raise ValueError("q8_matmul: res must be contiguous bf16 [M,N]")
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x2.device)
    rc = _lib.lib().vaa_model_q8_matmul(xq.data_ptr(), ascale.data_ptr(), outl.data_ptr(), x2.data_ptr(), M, codes.data_ptr(), wscale.data_ptr(), N, K,
                                        res.data_ptr() if res is not None else None, y.data_ptr(), 1 if M <= Q8_GEMV_MAX_ROWS else 2, _stream())
    _lib.check(rc, "vaa_model_q8_matmul")
    return y


class Q8Linear(QuantLinear):
    """A frozen bias-free linear layer held as int8 codes: buffers `codes` int8 [out,in] and `wscale` float32 [out], and the outlier
    threshold of its calls. There is no `weight`; `dequantize()` forms wdq."""

    quant_type = INT8

    def __init__(self, codes: torch.Tensor, wscale: torch.Tensor, threshold: float = 6.0):
        super().__init__()
        if not threshold >= 0 or threshold == float("inf"):
            raise ValueError("Q8Linear: the threshold must be finite and >= 0")
        self.threshold = float(threshold)
        self.register_buffer("codes", codes)
        self.register_buffer("wscale", wscale)

    @classmethod
    def from_weight(cls, w: torch.Tensor, threshold: float = 6.0) -> "Q8Linear":
        return cls(*quantize_q8(w), threshold)

    @property
    def in_features(self) -> int:
        return int(self.codes.shape[1])

    def dequantize(self) -> torch.Tensor:
        return dequantize_q8(self.codes, self.wscale)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, threshold={self.threshold:g}"

    def linear2d(self, x2, res=None, scratch=None, gemv=True):
        """q8_linear at the layer's threshold; `gemv` means nothing here: the matmul's form is chosen by the row count alone."""
        return q8_linear(x2, self, res, None, scratch)


class Q8LinearRows(_FusedRows, Q8Linear, buffers=("codes", "wscale"), settings=("threshold",)):
    """Rows of a fused Q8Linear. A scale belongs to one row, so the slice is exactly the projection's own codes."""


def q8_linear(x2: torch.Tensor, lin: Q8Linear, res: torch.Tensor | None = None, threshold: float | None = None,
              scratch: Q8Scratch | None = None) -> torch.Tensor:
    """The LLM.int8 product of include/vaa_model_ops.h for x2 [M,K]: the rows are quantised per call, multiplied as integers, rescaled by
    ascale[m] * wscale[n], and the columns where ANY of the M rows reaches `threshold` (default: the layer's) are carried in bf16 — so a
    row's result depends on the other rows of its call unless the threshold is 0. bf16 on a GPU: vaa_model_q8_act_quant +
    vaa_model_q8_matmul. Elsewhere (CPU plumbing tests): q8_linear_torch, the same arithmetic in torch."""
    t = lin.threshold if threshold is None else float(threshold)
    if x2.is_cuda and x2.dtype == torch.bfloat16 and not Q8_TORCH_ROUTE:
        if x2.shape[0] == 0:
            return torch.empty((0, lin.out_features), dtype=torch.bfloat16, device=x2.device)
        x2 = x2.contiguous()
        xq, ascale, outl = q8_act_quant(x2, t, scratch)
        return q8_matmul(xq, ascale, outl, x2, lin.codes, lin.wscale, None if res is None else res.contiguous())
    return q8_linear_torch(x2, lin.codes, lin.wscale, res, t).to(x2.dtype)


QUANT_ERROR = ("this model's Llama projections were quantised to {bits} by quantize_llm: it is inference only (predict_action / evaluate_patch); "
               "{what} needs the bf16 weights — build a second, unquantised model for training or for the no-cache decoding route")


def refuse_training(what: str, quant_type=None):
    raise RuntimeError(QUANT_ERROR.format(what=what, bits="int8" if quant_type == INT8 else "4 bits"))


PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


@torch.no_grad()
def quantize_llm(model, quant_type: str = "fp4", threshold: float = 6.0):
    """Replace, in place, the seven projections of every LlamaLayer by Q4Linear modules and drop their bf16 weights (and the layer's cached
    transposed / concatenated copies). q / k / v share one row-concatenated Q4Linear (`qkv_q4`), gate / up likewise (`gate_up_q4`): the
    decode step runs each group as one launch. Vision towers, projector, embeddings and lm_head are left as they are. Returns the model.
    quant_type "int8": the same seven projections become Q8Linear modules (fused groups `qkv_q8`, `gate_up_q8`) whose calls split outlier
    columns at `threshold` (transformers' llm_int8_threshold; 0: no split); `model.quant_type` then reads "int8"."""
    int8 = quant_type == INT8
    if not int8:
        table_values(quant_type)
    elif not threshold >= 0 or threshold == float("inf"):
        raise ValueError("quantize_llm: the int8 threshold must be finite and >= 0")
    if getattr(model, "quant_type", None):
        raise ValueError("quantize_llm: the model is quantised already")
    cfg = model.cfg
    scratch = Q8Scratch() if int8 else Q4Scratch(cfg.llm_mlp * cfg.llm_dim)
    suffix, rows_cls = ("_q8", Q8LinearRows) if int8 else ("_q4", Q4LinearRows)
    for layer in model.layers:
        def take(names):
            w = torch.cat([getattr(layer, n).weight.detach() for n in names], 0) if len(names) > 1 else getattr(layer, names[0]).weight.detach()
            rows = [getattr(layer, n).weight.shape[0] for n in names]
            for n in names:
                delattr(layer, n)
            return (Q8Linear.from_weight(w, threshold) if int8 else Q4Linear.from_weight(w, quant_type)), rows

        layer._wt_cache.clear()
        for fused, names in (("qkv" + suffix, ("q_proj", "k_proj", "v_proj")), ("gate_up" + suffix, ("gate_proj", "up_proj"))):
            parent, rows = take(names)
            setattr(layer, fused, parent)
            r0 = 0
            for n, r in zip(names, rows):
                setattr(layer, n, rows_cls(parent, r0, r))
                r0 += r
        for n in ("o_proj", "down_proj"):
            setattr(layer, n, take((n,))[0])
        layer.quant_type = quant_type
        layer._quant_scratch = scratch  # a Q4Scratch or a Q8Scratch, shared by all layers
        layer.projections = QuantProjections(layer, suffix)
    model.quant_type = quant_type
    return model


class QuantProjections:
    """The 4-bit and the int8 kind of a converted layer's inference projections (openvla_model.Bf16Projections is the bf16 kind): the fused
    groups `qkv_q4` / `gate_up_q4` (or `_q8`) and o_proj / down_proj, each through its format's product on 2-D rows with the residual as
    `res` and the model's shared scratch. 4-bit honours `gemv` (False in prefill, True in a decode step); int8 chooses by the row count."""

    def __init__(self, layer, suffix: str):
        self.layer, self.suffix = layer, suffix

    def _linear(self, name, x2, res, gemv):
        return getattr(self.layer, name).linear2d(x2, res, self.layer._quant_scratch, gemv)

    def qkv(self, h2, fused, gemv):
        return self._linear("qkv" + self.suffix, h2, None, gemv)

    def o(self, a2, res, gemv):
        return self._linear("o_proj", a2, res, gemv)

    def gate_up(self, h2, fused, gemv):
        gu = self._linear("gate_up" + self.suffix, h2, None, gemv)
        mlp = gu.shape[1] // 2
        return gu[:, :mlp], gu[:, mlp:]

    def down(self, y2, res, fused_mlp, gemv):
        return self._linear("down_proj", y2.contiguous(), res, gemv)


def llm_weight_bytes(model) -> int:
    """Bytes held by the Llama layers' parameters and buffers (what quantize_llm shrinks)."""
    seen, total = set(), 0
    for layer in model.layers:
        for t in list(layer.parameters()) + list(layer.buffers()):
            if t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
    return total
