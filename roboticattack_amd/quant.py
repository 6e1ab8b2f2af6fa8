"""4-bit block-quantised Llama projections for the evaluation path (include/vaa_model_ops.h states the format; csrc/vaa_quant.hip holds the
two kernels): what the reference's evaluation gets from `from_pretrained(..., load_in_4bit=True)` (experiments/robot/openvla_utils.py:43-51),
built here because bitsandbytes does not exist on this platform. Inference only: `predict_action` and `evaluate_patch` run on a quantised
model, the training entry points refuse it.

  quantize_q4 / dequantize_q4   the quantiser and its inverse in torch (CPU and GPU give the same codes: every comparison is exact)
  Q4Linear                      codes + absmax as buffers, the table, no `weight`
  quantize_llm                  the seven projections of every LlamaLayer -> Q4Linear; towers, projector, embeddings and lm_head stay bf16
  layer_prefill / layer_decode  the second route of LlamaLayer.prefill / decode_step: vaa_model_q4_gemv for at most GEMV_MAX_ROWS rows in a
                                decode step, vaa_model_q4_dequant into one shared scratch + the stock GEMM otherwise and always in prefill
Neither table could be compared with bitsandbytes in this image; the fp4 entries are stated from memory.
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


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def q4_dequant(codes: torch.Tensor, absmax: torch.Tensor, table, out: torch.Tensor | None = None) -> torch.Tensor:
    """The dequantised weight [N,K] bf16 through vaa_model_q4_dequant on a GPU (into `out`, a contiguous buffer of at least N*K bf16, when
    given), through dequantize_q4 elsewhere."""
    N, K = codes.shape[0], codes.shape[1] * 2
    if not _on_gpu(codes):
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


class Q4Linear(nn.Module):
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
    def out_features(self) -> int:
        return int(self.codes.shape[0])

    @property
    def in_features(self) -> int:
        return int(self.codes.shape[1]) * 2

    def dequantize(self) -> torch.Tensor:
        return dequantize_q4(self.codes, self.absmax, self.table)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, quant_type={self.quant_type}"

    @torch.no_grad()
    def forward(self, x, res=None, scratch=None, gemv=True):
        """bf16(res + x @ wq^T) on the last axis of x (inference only)."""
        y = q4_linear(x.reshape(-1, x.shape[-1]), self, None if res is None else res.reshape(-1, self.out_features), scratch, gemv)
        return y.view(*x.shape[:-1], self.out_features)


class Q4LinearRows(Q4Linear):
    """Rows [row0, row0 + rows) of a fused Q4Linear (q / k / v of the row-concatenated qkv codes, gate / up likewise): the projection as a
    module of its own without a second copy of its codes. Blocks never cross a row, so the slice is exactly the projection's own codes."""

    def __init__(self, parent: Q4Linear, row0: int, rows: int):
        nn.Module.__init__(self)
        self.quant_type, self.table = parent.quant_type, parent.table
        self._src = (parent,)  # in a tuple: the parent is registered once, on the layer
        self.row0, self.rows = int(row0), int(rows)

    @property
    def codes(self):
        return self._src[0].codes[self.row0:self.row0 + self.rows]

    @property
    def absmax(self):
        return self._src[0].absmax[self.row0:self.row0 + self.rows]


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
    if _on_gpu(x2) and x2.dtype == torch.bfloat16:
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


QUANT_ERROR = ("this model's Llama projections were quantised to 4 bits by quantize_llm: it is inference only (predict_action / evaluate_patch); "
               "{what} needs the bf16 weights — build a second, unquantised model for training or for the no-cache decoding route")


def refuse_training(what: str):
    raise RuntimeError(QUANT_ERROR.format(what=what))


PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


@torch.no_grad()
def quantize_llm(model, quant_type: str = "fp4"):
    """Replace, in place, the seven projections of every LlamaLayer by Q4Linear modules and drop their bf16 weights (and the layer's cached
    transposed / concatenated copies). q / k / v share one row-concatenated Q4Linear (`qkv_q4`), gate / up likewise (`gate_up_q4`): the
    decode step runs each group as one launch. Vision towers, projector, embeddings and lm_head are left as they are. Returns the model."""
    table_values(quant_type)
    if getattr(model, "q4", None):
        raise ValueError("quantize_llm: the model is quantised already")
    cfg = model.cfg
    scratch = Q4Scratch(cfg.llm_mlp * cfg.llm_dim)
    for layer in model.layers:
        def take(names):
            w = torch.cat([getattr(layer, n).weight.detach() for n in names], 0) if len(names) > 1 else getattr(layer, names[0]).weight.detach()
            rows = [getattr(layer, n).weight.shape[0] for n in names]
            for n in names:
                delattr(layer, n)
            return Q4Linear.from_weight(w, quant_type), rows

        layer._wt_cache.clear()
        for fused, names in (("qkv_q4", ("q_proj", "k_proj", "v_proj")), ("gate_up_q4", ("gate_proj", "up_proj"))):
            parent, rows = take(names)
            setattr(layer, fused, parent)
            r0 = 0
            for n, r in zip(names, rows):
                setattr(layer, n, Q4LinearRows(parent, r0, r))
                r0 += r
        for n in ("o_proj", "down_proj"):
            setattr(layer, n, take((n,))[0])
        layer.q4 = quant_type
        layer._q4_scratch = scratch
    model.q4 = quant_type
    return model


# ---- the second inference route of LlamaLayer (openvla_model.py dispatches here when layer.q4 is set) ----
def _tail(layer, x, a, fused, gemv):
    """o_proj + residual, RMSNorm, SwiGLU MLP + residual on [B,T,D], every projection through q4_linear (residuals as `res`)."""
    from . import model_ops

    B, T, D = x.shape
    sc = layer._q4_scratch
    x2 = q4_linear(a.reshape(-1, D), layer.o_proj, x.reshape(-1, D), sc, gemv)
    h = layer._infer_norm(layer.post_attention_layernorm, x2.view(B, T, D), fused).reshape(-1, D)
    gu = q4_linear(h, layer.gate_up_q4, None, sc, gemv)
    mlp = gu.shape[1] // 2
    g, u = gu[:, :mlp], gu[:, mlp:]
    if fused and (B * T * mlp) % 8 == 0:
        y = model_ops.SwiGLUFn.apply(g, u)
    else:
        y = F.silu(g) * u
    return q4_linear(y.contiguous(), layer.down_proj, x2, sc, gemv).view(B, T, D)


def _qkv(layer, x, fused, gemv):
    B, T, D = x.shape
    h = layer._infer_norm(layer.input_layernorm, x, fused).reshape(-1, D)
    return q4_linear(h, layer.qkv_q4, None, layer._q4_scratch, gemv).view(B, T, 3, layer.heads, D // layer.heads)


@torch.no_grad()
def layer_prefill(layer, x, rope_tab, cache):
    """LlamaLayer.prefill on a quantised layer: the same graph, the projections as vaa_model_q4_dequant + GEMM (always: T is a whole prompt)."""
    from . import model_ops
    from .openvla_model import _rope

    B, T, D = x.shape
    fused = layer._infer_fused(x)
    qkv = _qkv(layer, x, fused, gemv=False)
    cos, sin = rope_tab[0][:T], rope_tab[1][:T]
    if fused:
        q, k = model_ops.RopeFn.apply(qkv[:, :, 0], cos, sin), model_ops.RopeFn.apply(qkv[:, :, 1], cos, sin)
    else:
        c, s = (torch.cat([t, t], -1).to(x.dtype)[None, :, None, :] for t in (cos, sin))
        q, k = _rope(qkv[:, :, 0], qkv[:, :, 1], c, s)
    v = qkv[:, :, 2]
    if fused and model_ops.attention_enabled(q):
        a = model_ops.attention_fwd(q, k, v, True)[0]
    else:
        a = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True).transpose(1, 2)
    cache[0][:, :T] = k
    cache[1][:, :T] = v
    return _tail(layer, x, a.reshape(B, T, D), fused, gemv=False)


@torch.no_grad()
def layer_decode(layer, x, pos, rope_tab, cache):
    """LlamaLayer.decode_step on a quantised layer: q/k/v as ONE vaa_model_q4_gemv over the row-concatenated codes, attention_decode, o_proj and
    down_proj with the residual as the kernel's `res`, gate/up as one launch. More than GEMV_MAX_ROWS rows take dequant + GEMM."""
    from . import model_ops

    B, _, D = x.shape
    fused = layer._infer_fused(x)
    qkv = _qkv(layer, x, fused, gemv=True)[:, 0]  # [B,3,H,hd]
    a = model_ops.attention_decode(qkv[:, 0], qkv[:, 1], qkv[:, 2], cache[0], cache[1], pos, rope_tab[0], rope_tab[1])
    return _tail(layer, x, a.reshape(B, 1, D), fused, gemv=True)


def llm_weight_bytes(model) -> int:
    """Bytes held by the Llama layers' parameters and buffers (what quantize_llm shrinks)."""
    seen, total = set(), 0
    for layer in model.layers:
        for t in list(layer.parameters()) + list(layer.buffers()):
            if t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
    return total
