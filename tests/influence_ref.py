"""What the influence tests share (CPU and GPU; nothing here needs a GPU): exact integer operands, real-valued operands with softmax
residuals, the float32 bound of a value and the value-tolerant comparison of lists, the bar of the residuals, synthetic cluster banks with
planted label flips, and a tiny bank."""
import torch

from uvc_amd import compact_influence as CI
from uvc_amd import compact_ood as CO
from uvc_amd import compact_probe as CPR

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
U = 2.0 ** -24                                       # the unit roundoff of float32
INF = float("inf")


# ---- exact operands: features in [-3, 3], residuals in {-1, 0, 1}: |sf + 1| <= 9 D + 1, |sr| <= Cr, the product below 2^24 for Cr <= 1000 ----
def int_case(nq, n, D, Cr, seed):
    """(fq [nq, D], rq [nq, Cr], fb [n, D], rb [n, Cr]) float32 with integer entries; the residuals are sparse (most entries 0), so many
    pairs share a value and the order rule is exercised everywhere."""
    g = torch.Generator().manual_seed(seed)
    fq = torch.randint(-3, 4, (nq, D), generator=g).float()
    fb = torch.randint(-3, 4, (n, D), generator=g).float()
    keep = max(2.0 / Cr, 0.05)
    sparse = lambda rows: (torch.randint(-1, 2, (rows, Cr), generator=g) * (torch.rand(rows, Cr, generator=g) < keep)).float()
    return fq, sparse(nq), fb, sparse(n)


def padded(t, ld, poison):
    """``t``'s values as a view with row stride ``ld`` into a buffer filled with ``poison`` (what lies between the rows must not be read
    into a result)."""
    buf = torch.full((t.shape[0], ld), poison, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


# ---- real-valued operands -----------------------------------------------------------------------------------------------------------------
def real_case(nq, n, D, C, seed):
    """Unit-normal features and the float32 softmax residuals of random logits (scale 3), padded with zeros to a multiple of 8."""
    g = torch.Generator().manual_seed(seed)
    fq, fb = torch.randn(nq, D, generator=g), torch.randn(n, D, generator=g)
    Cr = (C + 7) // 8 * 8

    def res(rows):
        z = 3.0 * torch.randn(rows, C, generator=g)
        y = torch.randint(0, C, (rows,), generator=g)
        r = torch.zeros(rows, Cr)
        r[:, :C] = CI.reference_residuals(z, y, C, "label")[0].float()
        return r
    return fq, res(nq), fb, res(n)


def value_bound(fq, rq, fb, rb, bias=1.0):
    """float64 [nq, n]: 1.001 (D + Cr + 2) 2^-24 (sum_d |fq fb| + |bias|) sum_c |rq rb|, the float32 bound of (sf + bias) * sr for operands as
    given.  sf is a chain of D fmafs from +0: |sf^ - sf| <= D u F with F = sum |fq fb| (first order); likewise |sr^ - sr| <= Cr u R; the
    add and the multiply round once each.  With |sf + bias| <= A = F + |bias| and |sr| <= R the first-order error of the product is at most
    A (Cr u R) + (D u F) R + 2 u A R <= (D + Cr + 2) u A R -- the constant is 1 --, and 1.001 covers the products of errors: (D + Cr + 2) u
    <= 4.1e-4 at the widest operands (D = 1024, Cr = 4096)."""
    d = lambda t: t.double().abs()
    A = d(fq) @ d(fb).T + abs(float(bias))
    R = d(rq) @ d(rb).T
    return 1.001 * (fq.shape[1] + rq.shape[1] + 2) * U * A * R


def check_lists(fq, rq, fb, rb, got, k, bias=1.0, exclude=None):
    """The value-tolerant rule for ``got = ((pos_vals, pos_idx), (neg_vals, neg_idx))`` (either may be None) on real data, operands as the
    device read them: filled slots hold distinct valid rows, each value is within ``value_bound`` of its own pair's float64 value, the
    values are ordered (equal values by ascending row), and the j-th value is within the LARGEST bound of the query's row of the
    reference's j-th value -- an order statistic moves by at most the largest error of any pair.  Returns the worst error / bound of the two checks."""
    v = CI.reference_values(fq, rq, fb, rb, bias)
    bound = value_bound(fq, rq, fb, rb, bias)
    ref = CI.reference_influence(fq, rq, fb, rb, k, bias, exclude)
    n = fb.shape[0]
    kk = min(k, n - (0 if exclude is None else 1))
    worst = [0.0, 0.0]
    for which, lst in enumerate(got):
        if lst is None:
            continue
        vals, idx = lst[0].double().cpu(), lst[1].long().cpu()
        empty = -INF if which == 0 else INF
        assert vals.shape == (fq.shape[0], k) and idx.shape == vals.shape
        assert (idx[:, kk:] == -1).all() and (vals[:, kk:] == empty).all()
        li, lv = idx[:, :kk], vals[:, :kk]
        assert (li >= 0).all() and (li < n).all()
        assert all(len(set(r)) == kk for r in li.tolist())
        if exclude is not None:
            assert not (li == torch.as_tensor(exclude).long()[:, None]).any()
        own, own_b = v.gather(1, li), bound.gather(1, li)
        assert ((lv - own).abs() <= own_b).all(), float(((lv - own).abs() / own_b.clamp_min(1e-300)).max())
        worst[0] = max(worst[0], float(((lv - own).abs() / own_b.clamp_min(1e-300)).max()))
        s = lv if which == 0 else -lv
        assert (s[:, :-1] >= s[:, 1:]).all()
        tie = s[:, :-1] == s[:, 1:]
        assert (li[:, :-1][tie] < li[:, 1:][tie]).all()
        row_b = bound.max(dim=1, keepdim=True)[0]
        want = ref[which][0][:, :kk]
        assert ((lv - want).abs() <= row_b).all(), float(((lv - want).abs() / row_b).max())
        worst[1] = max(worst[1], float(((lv - want).abs() / row_b.clamp_min(1e-300)).max()))
    return worst


# ---- the residuals' bar ---------------------------------------------------------------------------------------------------------------------
def residual_bars(logits, labels, classes, target, eps):
    """``(r, t, rsq, bar_r, bar_rsq)``: the float64 spec and the bars of the float32 results, from the spec.  The kernel forms d_c = z_c - max
    in float32 (relative error u), e_c = expf(d_c) (relative error at most ``eps``, measured), a float64 sum S, p_c = e_c / S in float64 and
    rounds the residual once.  To first order p^_c = p_c (1 + eta_c + d_c delta_c - sum_j p_j (eta_j + d_j delta_j)), so
        |r^_c - r_c| <= p_c (2 eps + u (|d_c| + sum_j p_j |d_j|)) 1.01 + u |r_c| + 1e-37
    (1.01: the products of errors; 1e-37: exponentials below the normal range).  rsq is the float64 sum of the squares of the STORED values:
    |rsq^ - rsq| <= sum_c (2 |r_c| bar_c + bar_c^2) + u rsq."""
    C = int(classes)
    z = logits.float()[:, :C].double()
    r, t, rsq = CI.reference_residuals(logits, labels, C, target)
    d = z - z.max(dim=1, keepdim=True)[0]
    p = torch.softmax(z, dim=1)
    pd = torch.where(p > 0, p * d.abs(), torch.zeros_like(p))
    bar = 1.01 * (p * (2 * eps) + U * (pd + p * pd.sum(dim=1, keepdim=True))) + U * r.abs() + 1e-37
    bar = torch.where((t >= 0)[:, None], bar, torch.zeros_like(bar))
    return r, t, rsq, bar, (2 * r.abs() * bar + bar * bar).sum(dim=1) + U * rsq


# ---- banks ------------------------------------------------------------------------------------------------------------------------------------
def make_bank(features, logits, labels, classes):
    return CO.make_ood_bank(features, logits, labels, classes, img_size=32, dataset="cifar10", split="train", interpolation="bilinear", crop_pct=None,
                            precision="fp32")


def tiny_banks(n=40, nq=7, D=16, C=5, seed=0):
    """(train bank, query bank): random features and logits of a head of 8 rows (the last three are padding)."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda rows: make_bank(torch.randn(rows, D, generator=g), torch.randn(rows, 8, generator=g), torch.randint(0, C, (rows,), generator=g), C)
    return mk(n), mk(nq)


def cluster_bank(n=600, D=16, C=4, sep=6.0, flips=0.05, seed=0, l2=1e-3):
    """A bank of C well-separated Gaussian clusters (centres ``sep`` e_c, unit noise) in which ``flips`` of the labels were moved to the
    next class, with the logits of a head fitted ON THE FLIPPED LABELS by ``compact_probe.fit_probe`` (float64, the CPU evaluator):
    ``(bank, flipped rows int64, ascending)``."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(n) % C
    x = torch.randn(n, D, generator=g)
    x[torch.arange(n), y] += sep
    bad = torch.sort(torch.randperm(n, generator=g)[:int(round(flips * n))])[0]
    yf = y.clone()
    yf[bad] = (y[bad] + 1) % C
    fit = CPR.fit_probe(x.double(), yf, C, l2, evaluator=CPR.reference_objective, max_iter=200)
    z = torch.zeros(n, 8)
    z[:, :C] = (x.double() @ fit["W"].T + fit["b"]).float()
    z[:, C:] = -1e4
    return make_bank(x, z, yf, C), bad
