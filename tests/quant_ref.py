"""What the 4-bit tests share (a plain module, not a conftest): an independent numpy restatement of the format of include/vaa_model_ops.h —
quantise (nearest table entry by exhaustive distance in fp64, ties to the smaller index), pack, the dequantised weight, and
y64 = res + x . wq^T in fp64 — plus the bound of the GEMV tests and the inputs they use. Nothing here imports roboticattack_amd.quant.

Exactness of the exhaustive search: the quotient and the table entries are fp32 numbers, their fp64 difference is rounded monotonically, so
the order of the distances is kept; a tie can only be manufactured by rounding between two candidates that are both far from the quotient
compared with its nearest neighbours' gap, never between the two nearest (those differences are exact: both operands within a factor of
2^29 of each other or one of them 0, which both tables hold).
"""
import numpy as np

BLOCK = 64
NF4 = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=np.float32)
_MAG = np.array([0.0, 1.0 / 192.0, 2.0 / 3.0, 1.0, 1.0 / 3.0, 0.5, 1.0 / 6.0, 0.25], dtype=np.float64)
FP4 = np.concatenate([_MAG, -_MAG]).astype(np.float32)
TABLES = {"nf4": NF4, "fp4": FP4}
GEMV_CHUNK_K = 1024  # one round of a vaa_model_q4_gemv workgroup over K (8 waves x 128 elements)
GEMV_ROWS = 16       # rows n per workgroup


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(f):
    """Round-to-nearest-even on finite fp32 values."""
    u = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_bf16(f):
    return bf16_bits_to_f32(f32_to_bf16_bits(f))


def quantise(w, table):
    """w fp32 [N,K] (bf16 values) -> (q uint8 [N,K], absmax fp32 [N,K/64])."""
    w = np.asarray(w, dtype=np.float32)
    N, K = w.shape
    blocks = w.reshape(N, K // BLOCK, BLOCK)
    absmax = np.abs(blocks).max(-1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (blocks / absmax[..., None]).astype(np.float32)  # numpy's fp32 division is IEEE
    dist = np.abs(table.astype(np.float64)[None, None, None, :] - quot.astype(np.float64)[..., None])
    q = dist.argmin(-1)  # the FIRST minimum: ties go to the smaller index
    zero = int(np.flatnonzero(table == 0)[0])
    q = np.where(absmax[..., None] == 0, zero, q)
    return q.reshape(N, K).astype(np.uint8), absmax


def pack(q):
    return ((q[:, 0::2] << 4) | q[:, 1::2]).astype(np.uint8)


def unpack(codes):
    return np.stack([codes >> 4, codes & 15], -1).reshape(codes.shape[0], -1)


def dequantise(q, absmax, table):
    """wq as fp32 holding bf16 values: ONE fp32 product, rounded to bf16 once."""
    prod = table[q].astype(np.float32) * np.repeat(absmax, BLOCK, axis=1).astype(np.float32)
    return round_bf16(prod.astype(np.float32))


def y64(x, wq, res=None):
    y = x.astype(np.float64) @ wq.astype(np.float64).T
    return y if res is None else y + res.astype(np.float64)


def gemv_bound(x, wq, ref):
    """|y - y64| <= 2^-8 |y64| + K 2^-23 sum_k |x_k wq_k|: one bf16 rounding plus a plain fp32 accumulation bound."""
    K = x.shape[1]
    return 2.0 ** -8 * np.abs(ref) + K * 2.0 ** -23 * (np.abs(x.astype(np.float64)) @ np.abs(wq.astype(np.float64)).T)


def random_bf16(rs, shape, scale=1.0):
    return round_bf16((rs.standard_normal(shape) * scale).astype(np.float32))


def gemv_case(M, N, K, table, seed=0):
    """(x, codes, absmax, wq, res) as numpy arrays: x / res / wq fp32 holding bf16 values. The kernels take any codes and scales, so these are
    drawn directly: uniform code bytes, log-uniform fp32 scales (not bf16 numbers: the product's rounding matters). The first block of row 0
    has absmax 0 and the last row of x is all zeros when M > 1."""
    rs = np.random.RandomState(seed * 7919 + M * 131 + N * 17 + K)
    codes = rs.randint(0, 256, size=(N, K // 2)).astype(np.uint8)
    absmax = np.exp(rs.uniform(-5.0, -1.0, size=(N, K // BLOCK))).astype(np.float32)
    absmax[0, 0] = 0.0
    x = random_bf16(rs, (M, K))
    if M > 1:
        x[-1] = 0.0
    return x, codes, absmax, dequantise(unpack(codes), absmax, table), random_bf16(rs, (M, N))
