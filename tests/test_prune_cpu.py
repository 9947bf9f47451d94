"""CPU: uvc_amd/compact_prune.py without a device -- the written spec of the gate gradients against the weight form, ``shrink`` against
``export_compact`` of the re-masked dense model, ``plan_removal`` against a brute-force restatement, the planted dead units, the ``apply``
command, the parsers' refusals and the ctypes rows of the new entry points."""
import ctypes
import json
import os
import re

import pytest
import torch

import attribution_ref as AR
import prune_ref as PF
from uvc_amd import compact as CP
from uvc_amd import compact_prune as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edge():
    """(dense state with masks, its export): HEAD_DIMS / UNITS of prune_ref"""
    sd = PF.edge_state()
    ex = CP.export_compact(sd)
    assert [[len(v) for v in b["v_index"]] for b in ex["blocks"]] == [[40, 20, 10], [64, 64], [16, 16, 16]]
    assert [(b["v_dim"], len(b["hidden_index"]), b["hidden"]) for b in ex["blocks"]] == [(48, 200, 256), (64, 130, 192), (16, 65, 128)]
    return sd, ex


# ---- the spec ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PF.EXPORTS)
def test_reference_gate_grads_equal_the_weight_form(name):
    """d L / d gamma at gamma = 1 of a gate that scales weight columns is sum_d W[d, cols] dW[d, cols]: float64, per image, 1e-12 of the
    largest entry; padding units are exact zeros; the table has the columns of the real candidates."""
    ex, x = AR.export_of(name)
    x = x.double()
    y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
    logits, loss, s = PR.reference_gate_grads(ex, x, y, nl, padded=True)
    want = PF.weight_form(ex, x, y, nl)
    G, real, pad = PR._columns(ex)
    assert s.shape == want.shape == (x.shape[0], G) and len(real) == len(PR.gate_table(ex))
    e = float((s - want).abs().max() / want.abs().max())
    print(f"{name}: gate form against weight form {e:.3e} of the largest entry {float(want.abs().max()):.3e}; {len(pad)} padding units")
    assert e <= 1e-12
    assert not bool(s[:, pad].any())
    assert torch.equal(PR.reference_gate_grads(ex, x, y, nl)[2], s[:, real])
    z = CP.reference_forward(ex, x)
    assert float((logits - z).abs().max()) <= 1e-12 * float(z.abs().max())          # (per image against the batch: the summation order of the GEMMs)
    assert torch.allclose(loss, torch.logsumexp(z[:, :nl], 1) - z[torch.arange(len(y)), torch.tensor(y)], rtol=0, atol=1e-12)
    if name == "no_heads":
        assert [t for t in PR.gate_table(ex) if t[0] == 0 and t[1] == 1] == []
    with pytest.raises(ValueError, match="labels"):
        PR.reference_gate_grads(ex, x, [nl] * x.shape[0], nl)


# ---- shrink -----------------------------------------------------------------------------------------------------------------------------
REMOVALS = {
    "widest_head": {0: dict(heads=[0])},                                       # v_dim 48 -> 32
    "two_widest": {0: dict(heads=[0, 1])},                                     # v_dim 48 -> 16
    "all_heads": {1: dict(heads=[0, 1])},
    "all_units": {2: dict(units=list(range(65)))},
    "on_a_multiple": {0: dict(units=list(range(3, 3 + 72)))},                  # 200 -> 128 kept: hidden 128
    "one_past_a_multiple": {0: dict(units=list(range(5, 5 + 71)))},            # 200 -> 129 kept: hidden 192
    "mixed": {0: dict(heads=[2], units=[0, 199, 57]), 1: dict(heads=[1], units=list(range(0, 130, 2))), 2: dict(heads=[0, 1, 2], units=[64])},
    "nothing": {},
}
WIDTHS = {"widest_head": (0, 2, 32, 256), "two_widest": (0, 1, 16, 256), "all_heads": (1, 0, 0, 192), "all_units": (2, 3, 16, 0),
          "on_a_multiple": (0, 3, 48, 128), "one_past_a_multiple": (0, 3, 48, 192)}


@pytest.mark.parametrize("case", list(REMOVALS))
def test_shrink_equals_export_of_the_remasked_dense_model(edge, case):
    sd, ex = edge
    removal = REMOVALS[case]
    got = PR.shrink(ex, removal)
    want = CP.export_compact(PF.mask_removal(sd, ex, removal))
    assert PF.same_export(got, want), case
    assert CP.check_export(got) is got
    if case in WIDTHS:
        k, nh, dv, F = WIDTHS[case]
        b = got["blocks"][k]
        assert (len(b["heads"]), b["v_dim"], b["hidden"]) == (nh, dv, F)
    if case == "all_heads":
        assert got["state_dict"]["blocks.1.attn.proj.weight"].shape == (192, 0) and torch.equal(got["state_dict"]["blocks.1.attn.proj.bias"], ex["state_dict"]["blocks.1.attn.proj.bias"])
    if case == "all_units":
        assert got["state_dict"]["blocks.2.mlp.fc2.weight"].shape == (192, 0) and torch.equal(got["state_dict"]["blocks.2.mlp.fc2.bias"], ex["state_dict"]["blocks.2.mlp.fc2.bias"])
    # the forward: the source with the removed columns zeroed
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a, b = CP.reference_forward(got, x), CP.reference_forward(PF.zero_removed(ex, removal), x)
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert ex["blocks"][0]["v_dim"] == 48 and ex["state_dict"]["blocks.0.mlp.fc1.weight"].shape[0] == 256          # the source is not touched


def test_shrink_refuses_bad_removals(edge):
    _, ex = edge
    for bad, word in (({3: dict(heads=[0])}, "block"), ({0: dict(heads=[3])}, "head"), ({0: dict(units=[200])}, "unit"), ({0: dict(units=[1, 1])}, "unit"),
                      ({0: dict(head=[0])}, "keys")):
        with pytest.raises(ValueError, match=word):
            PR.shrink(ex, bad)


# ---- plan_removal -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(keep_macs=0.8, min_heads=1, min_units=64), dict(keep_macs=0.45, min_heads=0, min_units=0),
                                dict(keep_macs=0.78, min_heads=2, min_units=100, rank="per_mac"), dict(keep_macs=1.0, min_heads=1, min_units=64),
                                dict(keep_macs=0.6, min_heads=1, min_units=64, criterion="abs")])
def test_plan_equals_the_brute_force_restatement(edge, kw):
    _, ex = edge
    table = PR.gate_table(ex)
    key = PF.tied_keys(len(table))
    assert int((key == 0.5).sum()) * 4 >= len(table)
    scores = PF.fake_scores(ex, key)
    eff = PR.candidate_keys(ex, scores, kw.get("criterion", "taylor"), kw.get("rank", "raw"))
    if kw.get("rank") == "per_mac":
        cost = torch.tensor([PR.candidate_cost(ex, t[0], t[1]) for t in table], dtype=torch.float64)
        assert torch.equal(eff, key / cost)
        N, D = CP._seq(ex["cfg"]), 192
        assert PR.candidate_cost(ex, 0, 0) == N * D * (128 + 2 * 48) + N * N * (64 + 48) and PR.candidate_cost(ex, 1, 2) == 2 * N * D
    else:
        assert torch.equal(eff, key)
    source = CP.compact_macs(ex, padded=True)
    target = kw["keep_macs"] * source
    want, trace = PF.plan_brute(ex, eff, target, kw["min_heads"], kw["min_units"])
    got = PR.plan_removal(ex, scores, **kw)
    assert got == want
    assert got == PR.plan_removal(ex, scores, **kw)                                  # deterministic
    out = PR.shrink(ex, got)
    macs = CP.compact_macs(out, padded=True)
    assert macs == trace[-1] <= target and (len(trace) == 1 or trace[-2] > target)   # the stop point, and the fill leaves the padded MACs alone
    for k, b in enumerate(out["blocks"]):
        assert len(b["heads"]) >= min(kw["min_heads"], len(ex["blocks"][k]["heads"]))
        assert len(b["hidden_index"]) >= min(kw["min_units"], len(ex["blocks"][k]["hidden_index"]))
        if got[k]["units"]:
            assert len(b["hidden_index"]) == b["hidden"]                              # the fill: no padding slot left where a unit went
    print(f"{kw}: {len(trace) - 1} removals, padded MACs {source} -> {macs} (target {target:.0f}), removed "
          + " ".join(f"{len(r['heads'])}h/{len(r['units'])}u" for r in got.values()))
    if kw["keep_macs"] == 1.0:
        assert all(not r["heads"] and not r["units"] for r in got.values())


def test_plan_refusals_and_random(edge):
    _, ex = edge
    key = PF.tied_keys(len(PR.gate_table(ex)))
    scores = PF.fake_scores(ex, key)
    # the lowest value the floors leave reachable, named
    _, trace = PF.plan_brute(ex, key, 0, 1, 64)
    with pytest.raises(ValueError, match=f"lowest reachable value is {trace[-1]} "):
        PR.plan_removal(ex, scores, keep_macs=0.05)
    assert PR.plan_removal(ex, scores, target_macs=trace[-1])                         # ... and that value is reached
    other = CP.export_compact(PF.mask_removal(PF.edge_state(), ex, {0: dict(units=[0])}))
    with pytest.raises(ValueError, match="meta does not match"):
        PR.plan_removal(other, scores, keep_macs=0.8)
    with pytest.raises(ValueError, match="meta does not match"):
        PR.plan_removal(other, scores, keep_macs=0.8, criterion="magnitude")
    with pytest.raises(ValueError, match="needs scores"):
        PR.plan_removal(ex, None, keep_macs=0.8)
    for kw in (dict(), dict(keep_macs=0.5, target_macs=10), dict(keep_macs=0.0), dict(keep_macs=1.5), dict(keep_macs=0.5, criterion="l1"),
               dict(keep_macs=0.5, rank="mac"), dict(keep_macs=0.5, min_units=-1)):
        with pytest.raises(ValueError):
            PR.plan_removal(ex, scores, **kw)
    with pytest.raises(ValueError, match="uvc-compact-gates"):
        PR.check_scores(dict(format="other"))
    a, b, c = (PR.plan_removal(ex, None, keep_macs=0.7, criterion="random", seed=s) for s in (5, 5, 6))
    assert a == b and a != c
    perm = torch.randperm(len(key), generator=torch.Generator().manual_seed(5))
    assert torch.equal(PR.candidate_keys(ex, None, "random", seed=5)[perm], torch.arange(len(key), dtype=torch.float64))
    m = PR.candidate_keys(ex, None, "magnitude")
    w = ex["state_dict"]
    assert float(m[0]) == float(w["blocks.0.attn.proj.weight"][:, :48].double().pow(2).sum())
    assert float(m[3 + 7]) == float(w["blocks.0.mlp.fc2.weight"][:, 7].double().pow(2).sum())


def test_planted_dead_units_go_first(edge):
    """40 real units with a zero fc1 row and zero b1 (u = GELU(0) = 0) and an fc2 column a hundred times larger: their gate gradient is exactly
    0, so taylor and abs take them first, magnitude last; without them the network computes what it computed."""
    _, ex = edge
    planted = list(range(10, 50))
    sd = {k: v.clone() for k, v in ex["state_dict"].items()}
    sd["blocks.0.mlp.fc1.weight"][planted] = 0
    sd["blocks.0.mlp.fc1.bias"][planted] = 0
    sd["blocks.0.mlp.fc2.weight"][:, planted] *= 100
    ex2 = CP.with_state(ex, sd)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    y, nl = PF.labels_of(3, 16)
    scores = PR.reference_importance(ex2, [(x[:2], y[:2]), (x[2:], y[2:])], nl)
    assert scores["images"] == 3 and scores["format"] == "uvc-compact-gates" and scores["version"] == 1
    assert scores["meta"] == dict(blocks=PR._widths(ex2), img_size=32, num_labels=nl, precision="reference", loss="ce")
    table = PR.gate_table(ex2)
    assert scores["table"].dtype == torch.int32 and scores["table"].tolist() == [list(t) for t in table]
    cols = [table.index((1, 0, p)) for p in planted]
    for crit in ("taylor", "abs"):
        key = PR.candidate_keys(ex2, scores, crit)
        assert not bool(key[cols].any()) and int((key == 0).sum()) == 40
        order = sorted(range(len(table)), key=lambda c: (float(key[c]), table[c][1], table[c][0], table[c][2]))
        assert order[:40] == cols
        # one 64-unit step of block 0 down (200 kept of 256 -> 192): the first eight planted units and nothing else
        one_step = CP.compact_macs(ex2, padded=True) - 64 * PR.candidate_cost(ex2, 1, 0)
        rem = PR.plan_removal(ex2, scores, target_macs=one_step, criterion=crit, min_units=0)
        assert rem == {0: dict(heads=[], units=planted[:8]), 1: dict(heads=[], units=[]), 2: dict(heads=[], units=[])}
    s_all = PR.reference_gate_grads(ex2, x, y, nl)[2]
    sq, ab = torch.zeros(len(table), dtype=torch.float64), torch.zeros(len(table), dtype=torch.float64)
    for b in range(3):                                                           # one chain per candidate over the images, whatever the batches
        sq += s_all[b].float().double() ** 2
        ab += s_all[b].float().double().abs()
    assert torch.equal(scores["sum_sq"], sq) and torch.equal(scores["sum_abs"], ab)
    mag = PR.candidate_keys(ex2, None, "magnitude")
    assert sorted(torch.argsort(mag, descending=True)[:40].tolist()) == cols
    out = PR.shrink(ex2, {0: dict(units=planted)})
    assert len(out["blocks"][0]["hidden_index"]) == 160 and out["blocks"][0]["hidden"] == 192
    a, b = CP.reference_forward(out, x), CP.reference_forward(ex2, x)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


# ---- the commands -----------------------------------------------------------------------------------------------------------------------
APPLY_KEYS = ["criterion", "filled", "macs_after", "macs_before", "macs_padded_after", "macs_padded_before", "output", "rank", "removed", "result",
              "source", "target_macs"]


def test_apply_command(edge, tmp_path, capsys):
    _, ex = edge
    src, sc, dst = (str(tmp_path / n) for n in ("m.compact.pt", "scores.pt", "small.compact.pt"))
    torch.save(ex, src)
    scores = PF.fake_scores(ex, PF.tied_keys(len(PR.gate_table(ex))))
    torch.save(scores, sc)
    rec = PR.main(["apply", "--compact", src, "--scores", sc, "--keep_macs", "0.7", "--output", dst])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(rec)) and sorted(line) == APPLY_KEYS
    out = CP.load_compact(dst)
    want = PR.shrink(ex, PR.plan_removal(ex, scores, keep_macs=0.7))
    assert PF.same_export(out, want)
    assert line["source"] == CP._report(ex) and line["result"] == CP._report(out)
    assert line["macs_padded_after"] == CP.compact_macs(out, padded=True) <= 0.7 * line["macs_padded_before"]
    assert line["macs_after"] == CP.compact_macs(out, padded=False) < line["macs_before"]
    assert [r["block"] for r in line["removed"]] == [0, 1, 2] and sum(r["units"] for r in line["removed"]) > 0 and line["filled"] >= 0
    assert sorted(line["removed"][0]) == ["block", "heads", "units"]
    # criteria that need no scores; a target in MACs
    rec = PR.main(["apply", "--compact", src, "--target_macs", str(line["macs_padded_after"]), "--criterion", "magnitude", "--rank", "per_mac",
                   "--min_heads", "0", "--min_units", "0", "--output", dst])
    assert rec["macs_padded_after"] <= line["macs_padded_after"] and rec["criterion"] == "magnitude" and rec["rank"] == "per_mac"
    CP.load_compact(dst)
    other = str(tmp_path / "other.compact.pt")
    torch.save(PR.shrink(ex, {0: dict(units=[0])}), other)
    with pytest.raises(ValueError, match="meta does not match"):
        PR.main(["apply", "--compact", other, "--scores", sc, "--keep_macs", "0.7", "--output", dst])


@pytest.mark.parametrize("argv, word", [
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0"], "--keep_macs"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "1.5"], "--keep_macs"),
    (["apply", "--compact", "f", "--output", "o", "--target_macs", "0"], "--target_macs"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5", "--target_macs", "5"], "not allowed with"),
    (["apply", "--compact", "f", "--output", "o"], "--keep_macs"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5", "--min_units", "-1"], "--min_units"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5", "--min_heads", "-1"], "--min_heads"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5", "--criterion", "l1"], "--criterion"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5", "--rank", "mac"], "--rank"),
    (["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.5"], "--scores"),
    (["apply", "--compact", "f", "--keep_macs", "0.5", "--criterion", "random"], "--output"),
    (["score", "--compact", "f", "--output", "o", "--data_dir", "d", "--max_images", "0"], "--max_images"),
    (["score", "--compact", "f", "--output", "o", "--data_dir", "d", "--num_labels", "0"], "--num_labels"),
    (["score", "--compact", "f", "--output", "o", "--data_dir", "d", "--precision", "fp16"], "--precision"),
    (["score", "--compact", "f", "--data_dir", "d"], "--output"),
    (["score", "--compact", "f", "--output", "o"], "--data_dir"),
    (["prune"], "invalid choice"),
])
def test_parsers_refuse_by_name(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        PR.main(argv)
    assert e.value.code != 0
    assert word in (capsys.readouterr().err + str(e.value))


def test_score_flags_come_from_the_shared_block():
    args = PR.build_parser().parse_args(["score", "--compact", "f", "--output", "o", "--data_dir", "d"])
    assert (args.split, args.max_images, args.num_labels, args.precision, args.dataset, args.eval_batch_size) == ("train", 2048, None, "bf16", "imagenet", 64)
    assert {"packed_dir", "resident", "interpolation", "crop_pct", "num_workers"} <= set(vars(args))
    a = PR.build_parser().parse_args(["apply", "--compact", "f", "--output", "o", "--keep_macs", "0.8"])
    assert (a.criterion, a.rank, a.min_heads, a.min_units, a.seed, a.scores, a.target_macs) == ("taylor", "raw", 1, 64, 0, None, None)


# ---- the bindings -----------------------------------------------------------------------------------------------------------------------
def _params(header, pattern):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.findall(r"(?:int|int64_t)\s+(" + pattern + r")\s*\((.*?)\);", src, flags=re.S)


def test_ctypes_rows_match_the_headers():
    """ctypes passes an argument beyond ``argtypes`` as a C int: every new declaration against its binding, by count and by kind."""
    from uvc_amd import _lib
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    found = _params("uvc_kernels.h", r"uvc_gate_dots|uvc_gate_accumulate")
    assert sorted(n for n, _ in found) == ["uvc_gate_accumulate", "uvc_gate_dots"]
    for name, params in found:
        want = [ctypes.c_void_p if "*" in p else kinds[p.split()[0]] for p in (q.strip() for q in params.split(","))]
        assert _lib._SIGNATURES[name] == want, name
    lib = CP._bind()
    found = _params("uvc_vit.h", r"uvc_vit_compact_gate_grads\w*")
    assert sorted(n for n, _ in found) == ["uvc_vit_compact_gate_grads", "uvc_vit_compact_gate_grads_workspace_bytes"]
    for name, params in found:
        got = getattr(lib, name).argtypes
        ps = [q.strip() for q in params.split(",")]
        assert len(got) == len(ps), name
        for g, p in zip(got, ps):
            if "*" in p:
                assert g is ctypes.c_void_p or issubclass(g, ctypes._Pointer), (name, p)
            else:
                assert g is kinds[p.split()[0]], (name, p)
        assert getattr(lib, name).restype is (ctypes.c_int64 if name.endswith("workspace_bytes") else ctypes.c_int)
    assert {"uvc_vit_compact_gate_grads", "uvc_vit_compact_gate_grads_workspace_bytes", "uvc_gate_dots", "uvc_gate_accumulate"} <= set(_lib.exported_symbols())
