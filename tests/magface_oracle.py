"""MagFace (Meng et al., CVPR 2021) in float64 numpy, written from the formulas and independently of the package: the forward, the
criterion, and the ANALYTIC gradients d L / d cos, d L / d a (a = the embedding's length), d L / d x and d L / d W.  No autograd.

Per row i: a_i = clamp(|x_i|, l_a, u_a); m_i = (u_m - l_m) / (u_a - l_a) * (a_i - l_a) + l_m; c = the target's class cosine clamped to
[-1, 1]; phi = c cos m_i - sqrt(1 - c^2) sin m_i; the target's value is phi where c > 0 else c (easy), or phi where c > cos(pi - m_i)
else c - m_i sin m_i (hard); logits = s * that on the target column, s * clamp(c_ij, -1, 1) elsewhere;
L = criterion(logits) + lambda_g * mean_i g(a_i), g(a) = a / u_a^2 + 1 / a ('sum': lambda_g * sum_i g(a_i)).

Conventions at the points where a derivative is one-sided: |x| equal to l_a or u_a and a cosine equal to -1 or 1 count as INSIDE the
clamp (torch.clamp's autograd passes the gradient there); at c = +-1 the derivative of sqrt(1 - c^2) is taken as 0, so d phi / d c =
cos m there (the ArcFace row kernel's convention; autograd gives inf)."""
import numpy as np

DEFAULTS = dict(s=64.0, l_a=10.0, u_a=110.0, l_m=0.45, u_m=0.8, lambda_g=35.0, easy_margin=True)


def f64(t):
    return np.asarray(t.detach().cpu().double().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def margins(norm, l_a, u_a, l_m, u_m):
    """|x| [B] -> dict(a, m, dm = d m / d |x|, g, dg = d g / d |x|, inside)"""
    norm = f64(norm)
    inside = (norm >= l_a) & (norm <= u_a)
    a = np.clip(norm, l_a, u_a)
    slope = (u_m - l_m) / (u_a - l_a)
    return dict(a=a, m=slope * (a - l_a) + l_m, dm=np.where(inside, slope, 0.0), g=a / u_a ** 2 + 1.0 / a,
                dg=np.where(inside, 1.0 / u_a ** 2 - 1.0 / a ** 2, 0.0), inside=inside)


def target(ct_raw, m, easy_margin):
    """target cosine [B] (raw), margins [B] -> (value, d value / d cos, d value / d m, took the margin branch)"""
    ct = np.clip(ct_raw, -1.0, 1.0)
    live = (ct_raw >= -1.0) & (ct_raw <= 1.0)
    sine = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    phi = ct * np.cos(m) - sine * np.sin(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        dphi = np.cos(m) + np.where(sine > 0.0, np.sin(m) * ct / np.where(sine > 0.0, sine, 1.0), 0.0)
    dphi_m = -(ct * np.sin(m) + sine * np.cos(m))
    if easy_margin:
        take = ct > 0.0
        val, dm = np.where(take, phi, ct), np.where(take, dphi_m, 0.0)
    else:
        take = ct > np.cos(np.pi - m)
        val, dm = np.where(take, phi, ct - m * np.sin(m)), np.where(take, dphi_m, -(np.sin(m) + m * np.cos(m)))
    return val, np.where(live, np.where(take, dphi, 1.0), 0.0), dm, take


def criterion(logits, label, gamma=0.0, weight=None, smoothing=0.0, reduction="mean"):
    """-> (loss_rows [B], scalar criterion loss, d loss / d logits [B, C]).  gamma: FocalLoss's mean((1 - p)^gamma * CE); weight /
    smoothing / reduction: nn.CrossEntropyLoss (its 'mean' divides by the sum of the targets' weights)"""
    B, C = logits.shape
    rows = np.arange(B)
    mx = logits.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))[:, 0]
    p = np.exp(logits - lse[:, None])
    hot = np.zeros_like(logits)
    hot[rows, label] = 1.0
    if weight is None and smoothing == 0.0 and reduction == "mean":
        logp = lse - logits[rows, label]
        pt = np.exp(-logp)
        om = np.maximum(1.0 - pt, 0.0)
        loss_rows = om ** gamma * logp
        f = om ** gamma + (gamma * logp * pt * om ** (gamma - 1.0) if gamma != 0.0 else 0.0)
        return loss_rows, loss_rows.mean(), f[:, None] * (p - hot) / B
    assert gamma == 0.0
    w = np.ones(C) if weight is None else f64(weight)
    wt, W, e = w[label], w.sum(), smoothing
    loss_rows = (1.0 - e) * wt * (lse - logits[rows, label]) + e / C * (W * lse - logits @ w)
    S = (1.0 - e) * wt + e / C * W
    d = S[:, None] * p - (1.0 - e) * wt[:, None] * hot - e / C * w[None, :]
    denom = 1.0 if reduction == "sum" else wt.sum()
    return loss_rows, loss_rows.sum() / denom, d / denom


def head(cos, label, norm, s=64.0, l_a=10.0, u_a=110.0, l_m=0.45, u_m=0.8, lambda_g=35.0, easy_margin=True, gamma=0.0, weight=None,
         smoothing=0.0, reduction="mean"):
    """class cosines [B, C] (raw, after pooling), labels, lengths [B] -> dict(logits, loss_rows, crit, reg, loss, dlogits, dcos,
    dnorm = d loss / d |x|, row_margin [B, 2], row_reg [B, 2])"""
    cos, label = f64(cos), np.asarray(label.cpu().numpy() if hasattr(label, "cpu") else label, dtype=np.int64)
    B, C = cos.shape
    rows = np.arange(B)
    mg = margins(norm, l_a, u_a, l_m, u_m)
    val, dval_c, dval_m, take = target(cos[rows, label], mg["m"], easy_margin)
    c = np.clip(cos, -1.0, 1.0)
    logits = s * c
    logits[rows, label] = s * val
    loss_rows, crit, dl = criterion(logits, label, gamma, weight, smoothing, reduction)
    k = 1.0 if reduction == "sum" else 1.0 / B
    reg = lambda_g * mg["g"].sum() * k
    dcos = dl * s * ((cos >= -1.0) & (cos <= 1.0))
    dcos[rows, label] = dl[rows, label] * s * dval_c
    dnorm = dl[rows, label] * s * dval_m * mg["dm"] + lambda_g * k * mg["dg"]
    return dict(logits=logits, loss_rows=loss_rows, crit=crit, reg=reg, loss=crit + reg, dlogits=dl, dcos=dcos, dnorm=dnorm, take=take,
                row_margin=np.stack([mg["m"], mg["dm"]], 1), row_reg=np.stack([mg["g"], mg["dg"]], 1), inside=mg["inside"])


def full(x, w, label, sub_centers=1, index=None, **kw):
    """embeddings [B, D], head weight [C * K, D], labels -> head()'s dict (over the pooled class cosines) plus demb [B, D] and
    dweight [C * K, D].  `index` (Partial FC): the sampled classes; `label` are then positions among them and the unsampled rows of
    dweight are 0."""
    x, w_all = f64(x), f64(w)
    K = sub_centers
    w_ = w_all if index is None else w_all[np.asarray(index, dtype=np.int64)]
    nx, nw = np.linalg.norm(x, axis=1), np.linalg.norm(w_, axis=1)
    xh, wh = x / nx[:, None], w_ / nw[:, None]
    cos_sub = xh @ wh.T
    B = x.shape[0]
    if K > 1:
        C = w_.shape[0] // K
        v = cos_sub.reshape(B, C, K)
        arg = v.argmax(2)                        # numpy's argmax: the lowest index among equals
        cos = np.take_along_axis(v, arg[..., None], 2)[..., 0]
    else:
        cos = cos_sub
    out = head(cos, label, nx, **kw)
    dcos = out["dcos"]
    if K > 1:
        dsub = np.zeros((B, C, K))
        np.put_along_axis(dsub, arg[..., None], dcos[..., None], 2)
        dcos = dsub.reshape(B, C * K)
    dxh, dwh = dcos @ wh, dcos.T @ xh
    out["demb"] = (dxh - xh * (xh * dxh).sum(1, keepdims=True)) / nx[:, None] + out["dnorm"][:, None] * xh
    dw = (dwh - wh * (wh * dwh).sum(1, keepdims=True)) / nw[:, None]
    if index is not None:
        dfull = np.zeros_like(w_all)
        dfull[np.asarray(index, dtype=np.int64)] = dw
        dw = dfull
    out["dweight"], out["cos"] = dw, cos
    return out
