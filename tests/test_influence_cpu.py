"""CPU: the written specs of ``uvc_amd.compact_influence`` -- the formula against autograd, the order and tie rules against a brute-force
loop, the refusals, planted label flips, and the three commands on tiny banks without a device."""
import json
import math

import numpy as np
import pytest
import torch

import influence_ref as IR
from uvc_amd import compact_influence as CI


def head_problem(n=9, nq=4, D=8, C=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(D, C).double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(C, D, generator=g))
        lin.bias.copy_(torch.randn(C, generator=g))
    fb, fq = torch.randn(n, D, generator=g).double(), torch.randn(nq, D, generator=g).double()
    yb, yq = torch.randint(0, C, (n,), generator=g), torch.randint(0, C, (nq,), generator=g)
    return lin, fb, yb, fq, yq


def grad_of(lin, f, y):
    """the gradient of the cross-entropy of ONE example with respect to (W, b), flattened"""
    loss = torch.nn.functional.cross_entropy(lin(f[None]), y[None])
    gw, gb = torch.autograd.grad(loss, [lin.weight, lin.bias])
    return torch.cat([gw.flatten(), gb.flatten()])


def test_the_formula_is_the_inner_product_of_autograd_gradients():
    lin, fb, yb, fq, yq = head_problem()
    C = lin.out_features
    with torch.no_grad():
        zb, zq = lin(fb).float(), lin(fq).float()                               # (the specs read float32 logits)
    gb = torch.stack([grad_of(lin, f, y) for f, y in zip(fb, yb)])                 # (float64 logits: compared at the rounding of z to float32)
    gq = torch.stack([grad_of(lin, f, y) for f, y in zip(fq, yq)])
    want = gq @ gb.T
    rb = CI.reference_residuals(zb, yb, C, "label")[0]
    rq = CI.reference_residuals(zq, yq, C, "label")[0]
    got = CI.reference_values(fq, rq, fb, rb)
    assert torch.allclose(got, want, rtol=0, atol=1e-5 * float(want.abs().max()))
    assert float(want.abs().max()) > 0.1
    # with float64 logits handed to the same formula: to rounding
    with torch.no_grad():
        pb, pq = torch.softmax(lin(fb), 1), torch.softmax(lin(fq), 1)
    pb[torch.arange(len(yb)), yb] -= 1
    pq[torch.arange(len(yq)), yq] -= 1
    assert torch.allclose(CI.reference_values(fq, pq, fb, pb), want, rtol=0, atol=1e-13)
    # the diagonal
    diag = (gb * gb).sum(1)
    si = CI.reference_self_influence(fb, zb, yb, C)
    assert torch.allclose(si, diag, rtol=1e-5, atol=0)
    assert torch.allclose(si, torch.diagonal(CI.reference_values(fb, rb, fb, rb)), rtol=1e-14, atol=0)


def test_residuals_targets_and_skipped_rows():
    z = torch.tensor([[1.0, 3.0, 3.0, -1e4], [0.0, 0.0, 0.0, 9.0], [2.0, -math.inf, 1.0, 0.0]])
    y = torch.tensor([0, 3, -1])
    r, t, rsq = CI.reference_residuals(z, y, 3, "label")
    assert t.tolist() == [0, -1, -1] and (r[1:] == 0).all() and rsq[1:].tolist() == [0.0, 0.0]
    p = torch.softmax(z[0, :3].double(), 0)
    assert torch.allclose(r[0], p - torch.tensor([1.0, 0, 0], dtype=torch.float64)) and abs(float(r[0].sum())) < 1e-15
    r, t, _ = CI.reference_residuals(z, None, 3, "pred")
    assert t.tolist() == [1, 0, 0]                                                 # the FIRST maximum among the valid columns
    assert float(r[2, 1]) == 0.0 and abs(float(r[2].sum())) < 1e-15
    with pytest.raises(ValueError, match="target"):
        CI.reference_residuals(z, y, 3, "other")


def brute_lists(v, k, exclude=None):
    """the lists by a loop: candidates sorted by (-v, row) / (v, row); NaN and the excluded row never enter"""
    pos, neg = [], []
    for q in range(v.shape[0]):
        cand = [(float(v[q, i]), i) for i in range(v.shape[1]) if not math.isnan(float(v[q, i])) and (exclude is None or exclude[q] != i)]
        pos.append(sorted(cand, key=lambda c: (-c[0], c[1]))[:k])
        neg.append(sorted(cand, key=lambda c: (c[0], c[1]))[:k])
    return pos, neg


@pytest.mark.parametrize("n,k", [(1, 3), (5, 5), (40, 1), (40, 7), (130, 64)])
def test_order_and_ties_against_a_brute_force_loop(n, k):
    fq, rq, fb, rb = IR.int_case(6, n, 8, 8, seed=n + k)
    fb[n // 2] = float("nan") if n > 4 else fb[n // 2]
    exclude = torch.tensor([0, -1, n - 1, 1 % n, -1, n + 5])
    for ex in (None, exclude):
        (pv, pi), (nv, ni) = CI.reference_influence(fq, rq, fb, rb, k, exclude=ex)
        v = CI.reference_values(fq, rq, fb, rb)
        bp, bn = brute_lists(v, k, None if ex is None else ex.tolist())
        for q in range(6):
            for vals, idx, want, empty in ((pv, pi, bp, -math.inf), (nv, ni, bn, math.inf)):
                m = len(want[q])
                assert idx[q, :m].tolist() == [i for _, i in want[q]] and vals[q, :m].tolist() == [x for x, _ in want[q]]
                assert (idx[q, m:] == -1).all() and (vals[q, m:] == empty).all()
    assert len({float(x) for x in v.flatten() if not math.isnan(float(x))}) < v.numel() / 2 or n < 5      # ties are plentiful


def test_refusals():
    train, query = IR.tiny_banks()
    with pytest.raises(ValueError, match="normalized"):
        CI.influence(dict(train, normalized=True), query, lists=CI.reference_lists)
    no_logits = {k: v for k, v in train.items() if k != "logits"}
    with pytest.raises(ValueError, match="no logits"):
        CI.influence(no_logits, query, lists=CI.reference_lists)
    with pytest.raises(ValueError, match="no logits"):
        CI.self_influence(no_logits, selfer=CI.reference_self_influence)
    other = IR.make_bank(torch.randn(3, 24), query["logits"][:3], query["labels"][:3], 5)
    with pytest.raises(ValueError, match="embed_dim 24 is not the train bank's embed_dim 16"):
        CI.influence(train, other, lists=CI.reference_lists)
    with pytest.raises(ValueError, match="data_classes 4 is not the train bank's data_classes 5"):
        CI.influence(train, dict(query, data_classes=4), lists=CI.reference_lists)
    with pytest.raises(ValueError, match="multiple of 8"):
        CI.self_influence(IR.make_bank(torch.randn(3, 12), query["logits"][:3], query["labels"][:3], 5), selfer=CI.reference_self_influence)
    for bad in (dict(k=0), dict(k=65), dict(rows=[7]), dict(rows=[]), dict(target="other"), dict(target=5)):
        with pytest.raises(ValueError):
            CI.influence(train, query, lists=CI.reference_lists, **bad)


def test_planted_flips_lead_the_self_influence_ranking():
    """600 rows in 4 clusters 6 sigma apart, 30 labels moved to the next class, the head fitted on the flipped labels by compact_probe's
    fitter.  The condition, fixed after the float64 reference met it on three seeds (and at separations 4 and 8): every one of the top 15
    rows (half the number of flips) is a flipped row.  (Measured: 29 of the top 30 are flipped rows at this separation.)"""
    for seed in (0, 1):
        bank, bad = IR.cluster_bank(sep=6.0, seed=seed)
        assert len(bad) == 30
        v = CI.self_influence(bank, selfer=CI.reference_self_influence)
        top = CI.rank_rows(v, bank["labels"], 4, 15)
        assert len(top) == 15 and set(top.tolist()) <= set(bad.tolist())
        per = CI.rank_rows(v, bank["labels"], 4, 3, per_class=True)
        assert len(per) == 12 and bank["labels"][per].tolist() == [c for c in range(4) for _ in range(3)]
        # a flipped row's proponents, when it is asked about under its (wrong) label, exclude itself and come from the label's class
        res = CI.influence(bank, bank, k=3, target="label", rows=bad[:4].tolist(), exclude=bad[:4], lists=CI.reference_lists, precision="fp32")
        assert not (res["pos_idx"] == bad[:4, None]).any()


def test_commands_run_on_tiny_banks_without_a_device(tmp_path, capsys):
    train, query = IR.tiny_banks()
    torch.save(train, tmp_path / "t.pt")
    torch.save(query, tmp_path / "q.pt")
    out = tmp_path / "infl.jsonl"
    line = CI.main(["explain", "--train_bank", str(tmp_path / "t.pt"), "--query_bank", str(tmp_path / "q.pt"), "--rows", "0", "3", "6", "--k", "4",
                    "--precision", "fp32", "--output", str(out)], lists=CI.reference_lists)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert set(line) == {"queries", "errors", "train_rows", "k", "target", "proponents_same_target", "opponents_other_label", "rows_per_s"}
    assert (line["queries"], line["errors"], line["train_rows"], line["k"], line["target"]) == (3, 0, 40, 4, "pred")
    recs = [json.loads(s) for s in out.read_text().splitlines()]
    assert [r["row"] for r in recs] == [0, 3, 6]
    res = CI.influence(train, query, k=4, rows=[0, 3, 6], precision="fp32", lists=CI.reference_lists)
    for j, r in enumerate(recs):
        assert set(r) == {"row"} | set(CI.RECORD_KEYS)
        assert r["pred"] == r["target"] == int(query["logits"][r["row"], :5].argmax()) and r["label"] == int(query["labels"][r["row"]])
        assert abs(r["prob"] - float(torch.softmax(query["logits"][r["row"], :5].double(), 0)[r["target"]])) < 1e-12
        for name, vals, idx in (("proponents", res["pos_vals"], res["pos_idx"]), ("opponents", res["neg_vals"], res["neg_idx"])):
            assert len(r[name]) == 4 and all(set(e) == {"row", "label", "value"} for e in r[name])
            assert [e["row"] for e in r[name]] == idx[j].tolist() and [e["value"] for e in r[name]] == vals[j].tolist()
            assert [e["label"] for e in r[name]] == train["labels"][idx[j]].tolist()
        assert r["proponents"][0]["value"] >= r["proponents"][-1]["value"] and r["opponents"][0]["value"] <= r["opponents"][-1]["value"]
    same = np.mean([e["label"] == r["target"] for r in recs for e in r["proponents"]])
    assert abs(line["proponents_same_target"] - same) < 1e-12
    # --target label, all rows, dicts instead of paths, stdout
    args = CI.build_parser().parse_args(["explain", "--train_bank", "x", "--query_bank", "y", "--target", "label", "--k", "64"])
    args.train_bank, args.query_bank = train, query
    line = CI.explain_command(args, lists=CI.reference_lists)
    printed = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()]
    assert line["queries"] == 7 == len(printed) and all(len(r["proponents"]) == 40 for r in printed)     # a bank of 40 rows fills 40 of 64 slots
    assert all(r["target"] == r["label"] for r in printed)
    # the refusals of the flag combinations
    for extra in (["--target_class", "1"], ["--compact", "f.pt"]):
        a = CI.build_parser().parse_args(["explain", "--train_bank", "x", "--query_bank", "y"] + extra)
        a.train_bank, a.query_bank = train, query
        with pytest.raises(ValueError):
            CI.explain_command(a, lists=CI.reference_lists)
    a = CI.build_parser().parse_args(["explain", "--train_bank", "x"])
    a.train_bank = train
    with pytest.raises(ValueError, match="--query_bank, or --compact and --images"):
        CI.explain_command(a, lists=CI.reference_lists)
    # self
    sus = tmp_path / "s.jsonl"
    line = CI.main(["self", "--bank", str(tmp_path / "t.pt"), "--top", "6", "--output", str(sus)], selfer=CI.reference_self_influence)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert set(line) == {"rows", "counted_rows", "written", "top", "per_class", "mean_value", "class_mean_value", "top_label_is_not_pred", "rows_per_s"}
    assert (line["rows"], line["counted_rows"], line["written"], line["top"], line["per_class"]) == (40, 40, 6, 6, 0)
    recs = [json.loads(s) for s in sus.read_text().splitlines()]
    v = CI.reference_self_influence(train["features"], train["logits"], train["labels"], 5)
    order = torch.sort(v, descending=True, stable=True).indices[:6]
    assert [r["row"] for r in recs] == order.tolist() and [r["value"] for r in recs] == v[order].tolist()
    assert all(tuple(r) == CI.SELF_KEYS for r in recs)
    assert len(line["class_mean_value"]) == 5
    for c in range(5):
        assert abs(line["class_mean_value"][c] - float(v[train["labels"] == c].mean())) < 1e-12
    assert abs(line["top_label_is_not_pred"] - np.mean([r["label"] != r["pred"] for r in recs])) < 1e-12
    line = CI.main(["self", "--bank", str(tmp_path / "t.pt"), "--top", "2", "--per_class", "1"], selfer=CI.reference_self_influence)
    printed = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()][:-1]
    assert line["written"] == 10 == len(printed) and [r["label"] for r in printed] == [c for c in range(5) for _ in range(2)]


def test_a_row_without_a_class_counts_for_nothing():
    train, query = IR.tiny_banks()
    train = dict(train, labels=train["labels"].clone())
    train["labels"][3], train["labels"][9] = -1, 5
    v = CI.self_influence(train, selfer=CI.reference_self_influence)
    assert float(v[3]) == 0.0 and float(v[9]) == 0.0
    assert not set(CI.rank_rows(v, train["labels"], 5, 40).tolist()) & {3, 9}
    res = CI.influence(train, query, k=40, lists=CI.reference_lists, precision="fp32")
    vals = torch.cat([res["pos_vals"], res["neg_vals"]], 1)
    idx = torch.cat([res["pos_idx"], res["neg_idx"]], 1)
    assert (vals[(idx == 3) | (idx == 9)] == 0).all()                              # a zero residual: influence 0 on everything
