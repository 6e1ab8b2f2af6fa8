"""fp64 reference of the K3 loss family (test infrastructure, no GPU): losses, prediction maps, gradients and a BOUND for every output.

What is computed
    The loss definitions are oracle/ref_port.py's (`uada_weighted_loss`, `upa_weighted_loss`, `cal_uad`, pinned to the reference's goldens) run on
    fp64 logits; `hf_ce` and `uada_weighted_loss` cast to fp32 inside, so they are restated here without the casts (`ce64`, `uada64`; test_loss_ref_host.py
    holds both restatements to ref_port's functions bit for bit on fp32 logits), and `upa_weighted_loss` runs with fp64 as the default dtype. The loops combine the terms as include/vaa.h cites them:
        UADA      w^2 MSE + 1 / CE          (UADA.py:145-148)           UADA_DDP  w^2 MSE                    (UADA_ddp.py:203-206)
        UPA       alpha angle + beta dist   (UPA.py:367-387)            CE        scale CE                   (TMA.py:148)
    Gradients are fp64 AUTOGRAD of that total with respect to the logits: no formula of csrc/vaa_rows_fold.h or oracle/vaa_oracle.c is repeated.
    Prediction maps are torch.argmax (first index on ties). The parameters {w, alpha, beta, scale} are rounded to fp32 first (the C-ABI passes
    floats); bf16 logits are rounded first and everything runs on the rounded values.

Layout
    The reference indexes logits [B,S,V] with S = n_img + L; here n_img = 0, S = L: row (b, k) predicts labels[b, k+1]. `rows` [R,V] holds the
    labelled rows in (b,k) row-major order (VAA_LAYOUT_ROWS); `to_full` scatters them into [B,S,V].

Bounds (computed in fp64 from the inputs, never from the code under test), u = 2^-23
    per row      A      = max(|z|_max of the row (finite entries), |lse|, |alse|)
                 d_ce   = 4 u A + 2^-21 (|lse| + |z_label|)                       the row's lse - z_label
                 d_E    = 4 u A sum_a p_a |a + 1 - E| + 2^-21 E                  the row's soft-argmax (second term 0 when every p_a but one is
                                                                                 exactly 0: a sum with one term is exact — UPA's e == l rows)
    scalars      every scalar is a function s(ce_1..R, E_1..R); d_s = sum |ds/dce_r| d_ce_r + sum |ds/dE_r| d_E_r + 2^-22 |s| (first-order
                 propagation by autograd; 2^-22: the fp32 store and one more rounding). UAD is exact decoding: 2^-22 |UAD|. Row counts are exact.
    gradient     g_i = kce (p_i - onehot_i) + kE p_a (a + 1 - E) with kce = d total / d ce_r, kE = d total / d E_r (autograd of s, used for the
                 bound only; `decomp_err` records that the decomposition reproduces the autograd gradient):
                     bound_i = 4 u A P_i + 2^-21 T_i + C_i
                     P_i = |kce| p_i + |kE| p_a |a + 1 - E|            T_i = |kce| (p_i + onehot_i) + |kE| p_a |a + 1 - E|
                     C_i = d_kce |p_i - onehot_i| + d_kE p_a |a + 1 - E| + |kE| p_a d_E
                 The first two terms are the rounding of z - lse (exp turns it into a relative error) and 4 fp32 ulps of the operands of the
                 final sum. C_i is the first-order propagation of the COEFFICIENTS' own bounds (d_kce, d_kE from d_ce, d_E through the second
                 derivatives of s, + 2^-22 of the coefficient) and of E inside (a + 1 - E): in the bins beside the soft-argmax p_a (a + 1 - E)
                 cancels and E's own error decides, and UADA's kce = -1 / (nrow CE^2) inherits 2 d_CE / CE. No fp32 evaluation avoids either:
                 the reference's own fp32 arithmetic breaks the first two terms alone by 5 to 160 x (test_loss_ref_host.py). For VAA_LOSS_CE
                 (kce = scale / nrow, no slice term) C_i is 2^-22 |g_i|.
                 bf16 outputs add 2^-8 |g_i| (one bf16 rounding, doubled). Where P_i > 0 the bound also carries 2^-126 (1 + |kce| + 256 |kE|): below the
                 smallest normal fp32 number a softmax term or the product may be flushed to zero (rows with logits 1e4 apart).
    An element whose bound is 0 (a column with p = 0, a row without the term) must be EXACTLY 0.

Not covered: the `nact == 0` batch. The reference's mse_loss over an empty selection is NaN, the kernels return 0; `loss_ref` returns 0 there and
nothing asserts either value. The B*L > 24576 global-label path of the FULL layout needs a tensor beyond a gigabyte and stays uncovered.
"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_port

A0, NA = 31744, 256
U = 2.0 ** -23
MODES = ("UADA", "UADA_DDP", "UPA", "CE")
MODE_ID = {"UADA": 0, "UADA_DDP": 1, "UPA": 2, "CE": 3}
SCALAR_NAMES = ("total", "CE", "MSE", "angle", "dist", "nrow", "nact", "UAD")
KW = dict(w=4.0, alpha=0.7, beta=0.3, scale=0.25)  # the parameters every test passes (none of them 1: a dropped factor shows)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def labelled(labels) -> list:
    """(b, k) of every labelled position in row-major order: row (b, k) predicts labels[b, k+1]."""
    lab = np.asarray(labels)
    B, L = lab.shape
    return [(b, k) for b in range(B) for k in range(L - 1) if lab[b, k + 1] != -100]


def to_full(rows: torch.Tensor, labels: torch.Tensor, S: int = None) -> torch.Tensor:
    """[R,V] labelled rows -> [B,S,V] (zeros elsewhere), row (b,k) at position S - L + k."""
    B, L = labels.shape
    S = L if S is None else S
    full = torch.zeros((B, S, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    rk = labelled(labels.cpu())
    if rk:
        full[torch.tensor([b for b, _ in rk]), torch.tensor([S - L + k for _, k in rk])] = rows
    return full


def ce64(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """ref_port.hf_ce (n_img = S - L) without its cast to fp32."""
    B, L = labels.shape
    n_img = logits.shape[1] - L
    mm = torch.cat([labels[:, :1], torch.full((B, n_img), -100, dtype=labels.dtype), labels[:, 1:]], dim=1)
    sl = logits[:, :-1, :].contiguous()
    tl = mm[:, 1:].contiguous()
    return F.cross_entropy(sl.view(-1, sl.shape[-1]), tl.view(-1), ignore_index=-100)


def uada64(logits: torch.Tensor, labels: torch.Tensor, mse_weight: float):
    """ref_port.uada_weighted_loss without its cast of the target to fp32 (autograd refuses an fp64 input against an fp32 target)."""
    temp_label = labels[:, 1:]
    action_mask = temp_label > 2
    action_logits = logits[:, :, A0 : A0 + NA][:, -temp_label.shape[-1] - 1 : -1, :][action_mask]
    reweigh = (torch.arange(1, 257) / 256).to(logits.dtype)
    r = (F.softmax(action_logits, dim=-1) * reweigh).sum(dim=-1)
    hard = temp_label[action_mask]
    hard[hard > 31872] = 31999
    hard[hard <= 31872] = 31744
    hard[hard == 31999] = 1 / 256  # truncates to 0 (Appendix A-D10), as in the reference
    hard[hard == 31744] = 1
    uad = ref_port.cal_uad(action_logits.argmax(dim=-1) + A0, temp_label[action_mask])
    return F.mse_loss(mse_weight * r.contiguous(), mse_weight * hard.to(r.dtype).contiguous()), uad


def upa64(logits, labels, alpha, beta):
    """ref_port.upa_weighted_loss with fp64 as the default dtype: its label coordinates `(int64 - 1) / 255` then divide in fp64, not fp32."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return ref_port.upa_weighted_loss(logits, labels, alpha, beta, logits.shape[1] - labels.shape[1])
    finally:
        torch.set_default_dtype(old)


def loss_terms(full: torch.Tensor, labels: torch.Tensor, mode: str, w, alpha, beta, scale) -> dict:
    """The reference's loss terms and the loop's total on logits [B,S,V] of any float dtype (fp64: the reference; fp32: its own arithmetic)."""
    zero = full.new_zeros(())
    nact = int((labels[:, 1:] > 2).sum())
    ce = ce64(full, labels) if full.dtype == torch.float64 else ref_port.hf_ce(full, labels, full.shape[1] - labels.shape[1])
    f64 = full.dtype == torch.float64
    mse, uad = (uada64 if f64 else ref_port.uada_weighted_loss)(full, labels, w) if nact > 0 else (zero, zero)
    out = dict(CE=ce, MSE=mse, UAD=uad, angle=zero, dist=zero)
    if mode == "UADA":
        out["total"] = mse + 1 / ce
    elif mode == "UADA_DDP":
        out["total"] = mse + 0
    elif mode == "UPA":
        tot, ang, dist = upa64(full, labels, alpha, beta) if f64 else ref_port.upa_weighted_loss(full, labels, alpha, beta, full.shape[1] - labels.shape[1])
        out.update(total=tot, angle=ang, dist=dist)
    else:
        out["total"] = scale * ce
    return out


def _from_row_stats(cer, E, lab, img, ords, B, mode, w, alpha, beta, scale) -> dict:
    """The same scalars as functions of the per-row statistics ce_r = lse - z_label and E_r (used for the bounds only)."""
    zero = cer.new_zeros(())
    CE = cer.mean()
    act = lab > 2
    t = torch.where(lab > 31872, 0.0, 1.0).to(cer.dtype)
    MSE = F.mse_loss(w * (E[act] / 256), w * t[act]) if bool(act.any()) else zero
    out = dict(CE=CE, MSE=MSE, angle=zero, dist=zero)
    if mode == "UADA":
        out["total"] = MSE + 1 / CE
    elif mode == "UADA_DDP":
        out["total"] = MSE + 0
    elif mode == "UPA":
        first = torch.stack([torch.nonzero((img == b) & (ords < 3)).flatten() for b in range(B)])  # [B,3] row indices
        e = (E[first] - 1) / 255
        l = ((lab[first] - 31743).to(cer.dtype) - 1) / 255
        ang = (F.cosine_similarity(e, l, dim=1) + 1).mean()
        dist = 1 / (torch.norm(e - l, p=2, dim=1).mean() + 1e-3)
        out.update(angle=ang, dist=dist, total=alpha * ang + beta * dist)
    else:
        out["total"] = scale * CE
    return out


def _prop(grads, deltas):
    """sum |d s / d x| d_x with 0 * (inf or nan) = 0: a statistic that is exact carries no error whatever the sensitivity."""
    tot = 0.0
    for g, d in zip(grads, deltas):
        term = torch.nan_to_num(g.abs(), nan=float("inf"), posinf=float("inf")) * d
        tot = tot + torch.where(d == 0, torch.zeros_like(d), term).sum(-1)
    return tot


class Ref(types.SimpleNamespace):
    def grad(self, layout: str, bf16: bool = False, S: int = None):
        """(gradient, bound) fp64 in layout FULL [B,S,V] | ROWS [R,V] | SLICE [R,256]; bf16: the output is stored as bf16."""
        g, b = self.g, self.gb + (2.0 ** -8 * self.g.abs() if bf16 else 0.0)
        if layout == "SLICE":
            return g[:, A0 : A0 + NA], b[:, A0 : A0 + NA]
        if layout == "FULL":
            return to_full(g, self.labels, S), to_full(b, self.labels, S)
        return g, b


def loss_ref(rows: torch.Tensor, labels: torch.Tensor, mode: str, w=5.0, alpha=0.8, beta=0.2, scale=1.0) -> Ref:
    """rows [R,V] (fp32 or bf16: the values the kernel reads), labels [B,L] int64 -> Ref (see the module docstring)."""
    w, alpha, beta, scale = (float(np.float32(x)) for x in (w, alpha, beta, scale))
    labels = labels.cpu()
    B, L = labels.shape
    z = rows.detach().cpu().double()
    R, V = z.shape
    rk = labelled(labels)
    assert len(rk) == R, (len(rk), R)
    lab = torch.tensor([int(labels[b, k + 1]) for b, k in rk])
    img = torch.tensor([b for b, _ in rk])
    ords = torch.tensor([sum(1 for (b2, k2) in rk if b2 == b and k2 < k) for b, k in rk])
    nact = int((lab > 2).sum())

    # ---- the reference on fp64 logits, gradient by autograd ----
    full = to_full(z, labels).requires_grad_(True)
    t = loss_terms(full, labels, mode, w, alpha, beta, scale)
    (gfull,) = torch.autograd.grad(t["total"], full)
    g = gfull[img, torch.tensor([k for _, k in rk])]
    assert float((gfull.abs().sum() - g.abs().sum()).abs()) <= 1e-12 * float(g.abs().sum()) + 1e-300  # nothing outside the labelled rows
    scalars = np.array([float(t["total"]), float(t["CE"]), float(t["MSE"]), float(t["angle"]), float(t["dist"]), R, nact, float(t["UAD"])])
    pred = np.full((B, L - 1), -1, np.int32)
    pred_full = np.full((B, L - 1), -1, np.int32)
    am, ams = torch.argmax(z, dim=1), torch.argmax(z[:, A0 : A0 + NA], dim=1)
    for i, (b, k) in enumerate(rk):
        pred_full[b, k] = int(am[i])
        if int(lab[i]) > 2:
            pred[b, k] = A0 + int(ams[i])

    # ---- row statistics and their bounds ----
    with torch.no_grad():
        lse = torch.logsumexp(z, dim=1)
        p = torch.exp(z - lse[:, None])
        zl = z[torch.arange(R), lab]
        zs = z[:, A0 : A0 + NA]
        alse = torch.logsumexp(zs, dim=1)
        pa = torch.exp(zs - alse[:, None])
        bins = torch.arange(1, NA + 1, dtype=torch.float64)
        E0 = (pa * bins).sum(1)
        dev = (bins[None, :] - E0[:, None]).abs()
        zmax = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z)).max(dim=1).values
        A = torch.maximum(torch.maximum(zmax, lse.abs()), alse.abs())
        d_ce = 4 * U * A + 2.0 ** -21 * (lse.abs() + zl.abs())
        several = ((pa > 0).sum(1) > 1).double()  # a sum with ONE non-zero term (every other exp underflows, in fp64 too) is exact
        d_E = 4 * U * A * (pa * dev).sum(1) + 2.0 ** -21 * E0 * several
        onehot = torch.zeros_like(z)
        onehot[torch.arange(R), lab] = 1.0
    cer = (lse - zl).clone().requires_grad_(True)
    E = E0.clone().requires_grad_(True)
    s = _from_row_stats(cer, E, lab, img, ords, B, mode, w, alpha, beta, scale)
    sb = np.zeros(8)
    for idx, key in ((0, "total"), (1, "CE"), (2, "MSE"), (3, "angle"), (4, "dist")):
        assert abs(float(s[key]) - scalars[idx]) <= 1e-11 * max(1.0, abs(scalars[idx])), (key, float(s[key]), scalars[idx])
        if s[key].requires_grad:
            gs = torch.autograd.grad(s[key], (cer, E), retain_graph=True, allow_unused=True)
            gs = [torch.zeros(R, dtype=torch.float64) if x is None else x for x in gs]
            sb[idx] = float(_prop(gs, (d_ce, d_E)))
        sb[idx] += 2.0 ** -22 * abs(scalars[idx])
    sb[7] = 2.0 ** -22 * abs(scalars[7])
    kk = torch.autograd.grad(s["total"], (cer, E), create_graph=True, allow_unused=True)
    kce, kE = [torch.zeros(R, dtype=torch.float64) if x is None else x for x in kk]
    d_k = []
    for kv in (kce, kE):
        dk = torch.zeros(R, dtype=torch.float64)
        for r in range(R):
            if kv.requires_grad:
                hs = torch.autograd.grad(kv[r], (cer, E), retain_graph=True, allow_unused=True)
                hs = [torch.zeros(R, dtype=torch.float64) if x is None else x for x in hs]
                dk[r] = _prop(hs, (d_ce, d_E))
        d_k.append(dk + 2.0 ** -22 * kv.detach().abs())
    kce, kE = kce.detach(), kE.detach()
    d_kce, d_kE = d_k
    with torch.no_grad():
        sl = pa * dev
        P = kce.abs()[:, None] * p
        P[:, A0 : A0 + NA] += kE.abs()[:, None] * sl
        T = P + kce.abs()[:, None] * onehot
        C = d_kce[:, None] * (p - onehot).abs()
        C[:, A0 : A0 + NA] += d_kE[:, None] * sl + kE.abs()[:, None] * pa * d_E[:, None]
        gb = 4 * U * A[:, None] * P + 2.0 ** -21 * T + C
        tiny = 2.0 ** -126 * (1.0 + kce.abs() + float(NA) * kE.abs())[:, None]  # fp32 has no normal number below 2^-126: p_i or the product may flush to 0
        gb = gb + torch.where(P > 0, tiny.expand_as(P), torch.zeros_like(P))
        gdec = kce[:, None] * (p - onehot)
        gdec[:, A0 : A0 + NA] += kE[:, None] * pa * (bins[None, :] - E0[:, None])
        decomp_err = float((gdec - g).abs().max()) / max(float(g.abs().max()), 1e-300)
    return Ref(mode=mode, labels=labels, rows=rk, lab=lab, scalars=scalars, scalars_bound=sb, pred=pred, pred_full=pred_full, g=g, gb=gb,
               decomp_err=decomp_err, stats=dict(lse=lse, E=E0, alse=alse, kce=kce, kE=kE, p=p, pa=pa, d_ce=d_ce, d_E=d_E, A=A))


def loss_ref_groups(rows: torch.Tensor, labels: torch.Tensor, P: int, mode: str, params: list) -> list:
    """Segmented forms: group g = images g*B/P .. with its own rows, means over its own images and rows; params[g] = dict(w, alpha, beta, scale)."""
    B = labels.shape[0]
    Bp = B // P
    out, r0 = [], 0
    for gidx in range(P):
        lg = labels[gidx * Bp : (gidx + 1) * Bp]
        n = len(labelled(lg))
        out.append(loss_ref(rows[r0 : r0 + n], lg, mode, **params[gidx]))
        r0 += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the comparison helper: every output of every form goes through here
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check(name: str, got, ref, bound) -> float:
    """|got - ref| <= bound element by element (bound 0: exactly equal). Returns the worst error / bound; raises with the worst element."""
    got = torch.as_tensor(np.asarray(got.detach().double().cpu()) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64))
    ref = torch.as_tensor(np.asarray(ref, np.float64)) if not isinstance(ref, torch.Tensor) else ref.double()
    bound = torch.as_tensor(np.asarray(bound, np.float64)) if not isinstance(bound, torch.Tensor) else bound.double()
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    ok = err <= bound  # NaN fails
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        i = int(torch.argmax(ratio.flatten()))
        idx = np.unravel_index(i, tuple(ratio.shape)) if ratio.dim() else ()
        raise AssertionError(f"{name}: element {tuple(int(x) for x in idx)} got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} "
                             f"err {float(err.flatten()[i]):.3e} bound {float(bound.flatten()[i]):.3e} (error / bound = {worst:.3g}; "
                             f"{int((~ok).sum())} of {ok.numel()} elements out)")
    return worst


def check_exact(name: str, got, ref) -> None:
    got, ref = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        i = np.argwhere(got != ref)[0]
        raise AssertionError(f"{name}: {int((got != ref).sum())} entries differ, first at {tuple(int(x) for x in i)}: got {got[tuple(i)]} ref {ref[tuple(i)]}")


def compare(ref: Ref, scalars=None, scalar_idx=range(8), pred=None, pred_full=None, grad=None, layout="ROWS", bf16=False, S=None, tag="") -> dict:
    """One K3 result against `ref`: scalars (the listed indices) and gradient within their bounds, the prediction maps exactly.
    Returns {output class: worst error / bound}."""
    out = {}
    if scalars is not None:
        idx = list(scalar_idx)
        sc = np.asarray(scalars.detach().double().cpu() if isinstance(scalars, torch.Tensor) else scalars, np.float64)
        for i in idx:  # one by one: the message names the scalar
            out["scalar:" + SCALAR_NAMES[i]] = check(f"{tag} scalars[{i}] ({SCALAR_NAMES[i]})", sc[i : i + 1], ref.scalars[i : i + 1], ref.scalars_bound[i : i + 1])
    if pred is not None:
        check_exact(f"{tag} pred_tokens", pred, ref.pred)
        out["pred"] = 0.0
    if pred_full is not None:
        check_exact(f"{tag} pred_full_tokens", pred_full, ref.pred_full)
        out["pred_full"] = 0.0
    if grad is not None:
        g, b = ref.grad(layout, bf16, S)
        out["grad"] = check(f"{tag} grad[{layout}{', bf16' if bf16 else ''}]", grad, g, b)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CASES: name -> Case(modes, dtypes, build(mode, dtype) -> (rows fp32 [R,V] holding values of `dtype`, labels [B,L]))
# ---------------------------------------------------------------------------------------------------------------------------------------------
L_DEF = 12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _actions(g, B):
    return torch.randint(A0, A0 + NA, (B, 7), generator=g)


def make_labels(toks: list, L: int = L_DEF) -> torch.Tensor:
    """One label row per entry of `toks` (a list of token ids, -100 = unlabelled), right-aligned as the collator leaves them."""
    lab = torch.full((len(toks), L), -100, dtype=torch.int64)
    for b, t in enumerate(toks):
        assert len(t) <= L - 1
        if len(t):
            lab[b, L - len(t) :] = torch.tensor(t, dtype=torch.int64)
    return lab


def mode_labels(actions: torch.Tensor, mode: str, maskidx=(0, 3), L: int = L_DEF) -> torch.Tensor:
    """The labels each loop hands K3: 7 action tokens + EOS, masked to `maskidx` (UADA / UADA_DDP: mask_labels, UADA.py:371-379), overwritten by a
    target vector (CE: TMA.py:124-129) or left whole (UPA's reverse-direction mode)."""
    lab = make_labels([list(map(int, a)) + [2] for a in actions], L)
    if mode == "UPA":
        return lab
    if mode == "CE":
        tgt = torch.tensor([int(actions[0, i]) if i in maskidx else -100 for i in range(7)] + [2])
        return ref_port.tma_target_labels(lab, tgt)
    return ref_port.mask_labels(lab.clone(), list(maskidx))


def gauss_rows(g, R, V=32064, scale=2.0, boost=3.0):
    z = torch.randn(R, V, generator=g) * scale
    z[:, A0 : A0 + NA] += torch.randn(R, NA, generator=g) * boost
    return z


def _finish(z, dtype):
    return bf16_round(z) if dtype == "bf16" else z


def _nrows(labels):
    return len(labelled(labels))


def _b_gauss(mode, dtype, seed=11):
    g = _gen(seed)
    labels = mode_labels(_actions(g, 2 if mode == "UPA" else 3), mode)
    return _finish(gauss_rows(g, _nrows(labels)), dtype), labels


def _b_offset(mode, dtype):
    g = _gen(12)
    labels = mode_labels(_actions(g, 2 if mode == "UPA" else 3), mode, (1, 2, 5))
    R = _nrows(labels)
    if dtype == "f32":
        return gauss_rows(g, R) + 3000.0, labels
    sign = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0)[:, None]  # bf16: one step is 64 at 1e4
    return bf16_round(gauss_rows(g, R, scale=40.0, boost=60.0) + 1e4 * sign), labels


def _b_confident(mode, dtype):
    g = _gen(13)
    labels = mode_labels(_actions(g, 3), mode, (0, 1, 2))
    # (scale 7: the other columns' mass sits in a few dozen terms. At scale 2 it is spread over all 32,063 and the reference's own fp32 sum of the
    # exponentials, a running total of 1 + many terms of 1e-6, is off by 9e-6 on a row: 1.13 x the bound. The case was ill-conditioned for fp32 eager.)
    # The low tail is cut at -4: z - lse of a column 33 below a maximum of 20 rounds twice at magnitude 2 A (z - max, then - log sum), which alone can
    # use up the 4 u A of the bound (measured on the untrimmed case: 1.01 x the bound on one element).
    z = _finish(gauss_rows(g, _nrows(labels), scale=7.0).clamp(min=-4.0), dtype)
    lab = torch.tensor([int(labels[b, k + 1]) for b, k in labelled(labels)])
    pl = torch.linspace(0.55, 0.97, z.shape[0])
    for r in range(z.shape[0]):
        z[r, lab[r]] = -float("inf")
        z[r, lab[r]] = torch.logsumexp(z[r].double(), 0).float() + torch.log(pl[r] / (1 - pl[r]))
    return _finish(z, dtype), labels


def _b_peaked(mode, dtype):
    g = _gen(14)
    labels = mode_labels(_actions(g, 2 if mode == "UPA" else 3), mode, (0, 1, 2))
    z = _finish(gauss_rows(g, _nrows(labels)), dtype)
    lab = torch.tensor([int(labels[b, k + 1]) for b, k in labelled(labels)])
    cols = torch.randint(0, NA, (z.shape[0],), generator=g)
    for r in range(z.shape[0]):
        # rows 0..2 (UPA: image 0's three coordinates): the label's own bin 2000 above everything -> e == l exactly (dn = 0);
        # the others: a random bin 60 above the slice -> E is an integer to fp32
        if r < 3 and int(lab[r]) > 2:
            z[r, lab[r]] = z[r].max() + 2000.0
        else:
            z[r, A0 + cols[r]] = z[r, A0 : A0 + NA].max() + 60.0
    return _finish(z, dtype), labels


TIE_SETS = [[8015, 8016], [16031, 16032], [24047, 24048], [0, 32063], [0, 8015, 8016, 16031, 16032, 24047, 24048, 32063],
            [3, 4], [1023, 1024], [2047, 2048, 4095, 4096], [8191, 8192], [8016, 8015 + 8016]]
SLICE_TIE_SETS = [[31744, 31751], [31751, 31752], [31752, 31999], [31744, 31751, 31752, 31999], [31999, 31744]]


def _b_ties(mode, dtype):
    g = _gen(15)
    labels = mode_labels(_actions(g, 2), "UPA")  # 16 rows in every mode: 7 action rows + the EOS row per image
    R = _nrows(labels)
    z = bf16_round(gauss_rows(g, R).clamp(max=4.0))  # every value exactly representable in bf16, in both precisions
    for r in range(R - 1):
        z[r, TIE_SETS[r % len(TIE_SETS)]] = 8.0
        st = SLICE_TIE_SETS[r % len(SLICE_TIE_SETS)]
        z[r, st] = 6.0 if r % 3 else 9.0  # every third row: the slice maxima are the row maxima too
    z[R - 1] = 1.0  # one all-equal row
    return z, labels


def _b_label_edges(mode, dtype):
    g = _gen(16)
    if mode == "UPA":  # the first three labels all 31744: l = 0, sqrt(nl) clamped at 1e-8
        a = _actions(g, 2)
        a[0, :3] = A0
        labels = mode_labels(a, "UPA")
    else:
        edge = [0, 8016, 24048, 31744, 31872, 31873, 31999, 32063]
        labels = torch.cat([make_labels([edge]), ref_port.mask_labels(make_labels([list(map(int, _actions(g, 1)[0])) + [2]]), [2, 4])])
    return _finish(gauss_rows(g, _nrows(labels)), dtype), labels


def _b_masked(mode, dtype):
    z, labels = _b_gauss(mode, "f32", seed=17)
    g = _gen(170)
    lab = torch.tensor([int(labels[b, k + 1]) for b, k in labelled(labels)])
    for r in range(z.shape[0]):
        cols = torch.randint(0, 32064, (500,), generator=g)
        cols = cols[((cols < A0) | (cols >= A0 + NA)) & (cols != lab[r])]
        z[r, cols] = -float("inf")
        z[r, 4096 + 64 * r : 4160 + 64 * r] = -float("inf")  # whole 16-byte vectors too (no label lives there)
    return z, labels


def _b_one_row(mode, dtype):
    g = _gen(18)
    labels = make_labels([[31900], []])  # R = 1; image 1 labels nothing
    return _finish(gauss_rows(g, 1), dtype), labels


def _b_wide(V):
    def build(mode, dtype):
        g = _gen(19 + V)
        labels = mode_labels(_actions(g, 2), mode, (0, 6))
        if mode == "CE":
            labels = labels.clone()
            labels[0, L_DEF - 1] = 39000  # a label beyond 32,767 (the EOS position of image 0)
        R = _nrows(labels)
        z = torch.randn(R, V, generator=g) * 2.0
        z[:, A0 : A0 + NA] += torch.randn(R, NA, generator=g) * 3.0
        z[0, V - 1] = 9.0  # the vocabulary argmax in the last column of the last part
        return _finish(z, dtype), labels
    return build


Case = types.SimpleNamespace
CASES = {
    "gauss": Case(modes=MODES, dtypes=("f32", "bf16"), V=32064, build=_b_gauss),
    "offset": Case(modes=MODES, dtypes=("f32", "bf16"), V=32064, build=_b_offset),
    "confident": Case(modes=("UADA", "CE"), dtypes=("f32", "bf16"), V=32064, build=_b_confident),
    "peaked_slice": Case(modes=("UADA", "UADA_DDP", "UPA"), dtypes=("f32", "bf16"), V=32064, build=_b_peaked),
    "ties": Case(modes=MODES, dtypes=("f32", "bf16"), V=32064, build=_b_ties),
    "label_edges": Case(modes=MODES, dtypes=("f32", "bf16"), V=32064, build=_b_label_edges),
    "masked_cols": Case(modes=MODES, dtypes=("f32",), V=32064, build=_b_masked),
    "one_row": Case(modes=("UADA", "UADA_DDP", "CE"), dtypes=("f32", "bf16"), V=32064, build=_b_one_row),
    "wide40": Case(modes=MODES, dtypes=("f32", "bf16"), V=40064, build=_b_wide(40064)),
    "wide64": Case(modes=MODES, dtypes=("f32", "bf16"), V=65536, build=_b_wide(65536)),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name: str, mode: str, dtype: str):
    rows, labels = CASES[name].build(mode, dtype)
    assert rows.shape[1] == CASES[name].V and rows.shape[0] == _nrows(labels) <= 40 and labels.shape[0] <= 4 and labels.shape[1] <= 12
    if dtype == "bf16":
        assert torch.equal(bf16_round(rows), rows)
    return rows, labels


@functools.lru_cache(maxsize=None)
def case_ref(name: str, mode: str, dtype: str) -> Ref:
    """The shared, cached reference of a case (computed once; callers do not modify it)."""
    rows, labels = case_inputs(name, mode, dtype)
    return loss_ref(rows, labels, mode, **KW)
