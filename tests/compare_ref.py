"""Operand families and helpers of the two-model comparison tests (tests/test_compare_cpu.py, tests/test_compare_gpu.py); nothing here
needs a GPU."""
import torch

from uvc_amd import compact_compare as CC

FAMILIES = ("normal", "close", "big", "tied", "sharp", "same")
_CACHE = {}


def pair(rows, C, lda, ldb, kind, seed):
    """(za float32 [rows, lda], zb float32 [rows, ldb]) on the host, seeded; columns [C, ld) hold NaN.
    normal: 3 randn, independent;  close: b = a + 0.05 randn (KL ~ 5e-3 at C = 1000);  big: magnitude 3e4;  tied: integers in [-2, 2]
    (every first-maximum and rank tie rule);  sharp: one column + 200 in each row, different columns in a and b wherever C > 1;
    same: b = a."""
    g = torch.Generator().manual_seed(seed)
    a, b = 3.0 * torch.randn(rows, C, generator=g), 3.0 * torch.randn(rows, C, generator=g)
    if kind == "close":
        b = a + 0.05 * torch.randn(rows, C, generator=g)
    elif kind == "big":
        a, b = (3e4 * torch.sign(t) + 10.0 * torch.randn(rows, C, generator=g) for t in (a, b))
    elif kind == "tied":
        a, b = (torch.randint(-2, 3, (rows, C), generator=g).float() for _ in range(2))
    elif kind == "sharp":
        ca = torch.randint(0, C, (rows,), generator=g)
        cb = (ca + 1 + torch.randint(0, max(C - 1, 1), (rows,), generator=g)) % C
        a[torch.arange(rows), ca] += 200.0
        b[torch.arange(rows), cb] += 200.0
    elif kind == "same":
        b = a.clone()
    elif kind != "normal":
        raise KeyError(kind)
    za, zb = torch.full((rows, lda), float("nan")), torch.full((rows, ldb), float("nan"))
    za[:, :C], zb[:, :C] = a, b
    return za.float().contiguous(), zb.float().contiguous()


def labels_for(rows, C, seed, dtype=torch.int64):
    """labels in [0, C) with -1 and C among them (rows 1, 4, 7 .. are -1 and rows 2, 7, 12 .. are C, where there are that many rows)"""
    y = torch.randint(0, C, (rows,), generator=torch.Generator().manual_seed(seed + 77))
    y[1::3] = -1
    y[2::5] = C
    return y.to(dtype)


def case(rows, C, lda, ldb, kind, seed):
    """(za, zb, labels int64, reference_pair_stats' dict, R float64 [rows]), built once per key and never changed: R is the larger of the
    two rows' max - min over the valid columns."""
    key = (rows, C, lda, ldb, kind, seed)
    if key not in _CACHE:
        za, zb = pair(rows, C, lda, ldb, kind, seed)
        y = labels_for(rows, C, seed)
        ref = CC.reference_pair_stats(za, zb, y, C)
        spread = lambda z: (z[:, :C].double().max(dim=1)[0] - z[:, :C].double().min(dim=1)[0])
        _CACHE[key] = (za, zb, y, ref, torch.maximum(spread(za), spread(zb)))
    return _CACHE[key]


def scale_of(name, ref, R):
    """The scale of the float bar: 1 for conf, tv and js; max(|ref|, R, 1) for kl_* and nll_*."""
    if name in ("conf_a", "conf_b", "tv", "js"):
        return torch.ones_like(R)
    return torch.maximum(torch.maximum(torch.nan_to_num(ref.abs(), nan=0.0), R), torch.ones_like(R))


def hand_banks():
    """Two 12-row, 3-class banks (num_classes 4 and 8, so the strides differ) whose every count is worked out in tests/test_compare_cpu.py.
    Row i: label, A's logits, B's logits."""
    rows = [
        (0, [5, 0, 0], [5, 0, 0]),       # both right
        (0, [5, 0, 0], [0, 5, 0]),       # a_only; moved 0 -> 1
        (0, [0, 3, 0], [3, 0, 0]),       # b_only
        (0, [0, 0, 5], [0, 0, 5]),       # neither
        (1, [0, 5, 0], [0, 5, 0]),       # both
        (1, [5, 0, 0], [0, 5, 0]),       # b_only; row 1's logits: a js tie, row 1 is listed first
        (1, [2, 2, 0], [2, 2, 0]),       # the label ties with column 0: the first maximum is column 0, the label has rank 1: neither
        (2, [0, 0, 5], [0, 0, 5]),       # both
        (2, [0, 0, 5], [0, 0, 5]),       # both
        (2, [1, 1, 1], [1, 1, 1]),       # all tied: the top-1 is column 0, the label has rank 2: neither
        (-1, [5, 0, 0], [5, 0, 0]),      # not counted; agrees
        (3, [0, 4, 0], [0, 0, 4]),       # not counted (label = C); disagrees, and each top-1 has rank 2 in the other row
    ]
    y = torch.tensor([r[0] for r in rows])
    za, zb = torch.full((12, 4), float("nan")), torch.full((12, 8), float("nan"))
    za[:, :3], zb[:, :3] = torch.tensor([r[1] for r in rows]).float(), torch.tensor([r[2] for r in rows]).float()
    mk = lambda z: dict(logits=z, labels=y.clone(), data_classes=3, num_classes=z.shape[1], meta={})
    return mk(za), mk(zb)


def same_record(rec, ref, rel=1e-12, path="record"):
    """asserts two records equal: keys, integers, strings, lists and None exactly; floats within ``rel`` of the larger magnitude (two ways of
    summing the same float64 terms)"""
    if isinstance(ref, dict):
        assert isinstance(rec, dict) and set(rec) == set(ref), (path, sorted(rec), sorted(ref))
        for k in ref:
            same_record(rec[k], ref[k], rel, f"{path}.{k}")
    elif isinstance(ref, list):
        assert isinstance(rec, list) and len(rec) == len(ref), path
        for j, (p, q) in enumerate(zip(rec, ref)):
            same_record(p, q, rel, f"{path}[{j}]")
    elif isinstance(ref, float) and isinstance(rec, float):
        assert abs(rec - ref) <= rel * max(abs(rec), abs(ref)), (path, rec, ref)
    else:
        assert type(rec) is type(ref) and rec == ref, (path, rec, ref)
