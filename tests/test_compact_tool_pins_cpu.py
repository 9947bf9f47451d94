"""CPU: the compact tools' command lines and bank dicts are what they were before their shared parts were merged
(uvc_amd/compact_tools.py, and ``add_image_file_flags`` in uvc_amd/compact.py): every action of every parser and subparser of the seven
tool modules and of ``compact predict`` / ``explain`` / ``attribute`` with its dest, type (and the bounds the type closes over), default,
choices, nargs, required and help, and the keys, ``meta``, dtypes and shapes of the four bank dicts, against
tests/golden/compact_tool_pins.json (recorded by tests/golden/make_compact_tool_pins.py before the merge).  Actions are matched by option
string: the order of unrelated flags in ``--help`` is free, nothing else is.  And the pieces that were merged stay merged."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "uvc_amd")
PARSERS = ["compact_transfer", "compact_transfer embed", "compact_transfer knn", "compact_transfer rehead", "compact_probe",
           "compact_probe embed", "compact_probe fit", "compact_probe score", "compact_calibrate", "compact_calibrate logits",
           "compact_calibrate fit", "compact_calibrate score", "compact_ood", "compact_ood bank", "compact_ood fit", "compact_ood score",
           "compact_robust", "compact_pixel", "compact_perturb", "compact predict", "compact explain", "compact attribute"]
BANKS = ["transfer", "probe_raw", "logits", "ood"]


@pytest.fixture(scope="module")
def pinned(request):
    sys.path.insert(0, GOLDEN)
    request.addfinalizer(lambda: sys.path.remove(GOLDEN))
    import make_compact_tool_pins as M
    now = dict(parsers={name: M.surface(p) for name, p in M.parsers().items()}, banks=M.banks())
    with open(os.path.join(GOLDEN, "compact_tool_pins.json")) as f:
        return json.loads(json.dumps(now)), json.load(f)


def _by_option(actions):
    """option string (the dest of a positional or of the subcommand) -> the action's record; no key twice."""
    out = {}
    for a in actions:
        for key in a["option_strings"] or [a["dest"]]:
            assert key not in out, key
            out[key] = a
    return out


def test_the_pins_cover_every_parser_and_bank(pinned):
    now, pins = pinned
    assert sorted(pins["parsers"]) == sorted(PARSERS) == sorted(now["parsers"])
    assert sorted(pins["banks"]) == sorted(BANKS) == sorted(now["banks"])


@pytest.mark.parametrize("name", PARSERS)
def test_parser_surface_is_the_pinned_one(pinned, name):
    now, pins = pinned
    got, want = _by_option(now["parsers"][name]), _by_option(pins["parsers"][name])
    assert sorted(got) == sorted(want)                                   # no action appears or disappears
    assert len(now["parsers"][name]) == len(pins["parsers"][name])
    for key in want:
        assert got[key] == want[key], key


@pytest.mark.parametrize("name", BANKS)
def test_bank_dict_is_the_pinned_one(pinned, name):
    now, pins = pinned
    assert now["banks"][name] == pins["banks"][name]


def _sources():
    return {f: open(os.path.join(PKG, f), encoding="utf-8").read() for f in sorted(os.listdir(PKG)) if f.endswith(".py")}


@pytest.mark.parametrize("text, count", [("torch.optim.LBFGS(", 1), ('"the loader yields no batch"', 1), ("need --data_dir or --packed_dir", 1),
                                         ('if k not in ("cfg", "state_dict", "blocks")', 1), ('("--packed_dir"', 2)])                  # (the drivers' block in driver.add_data_flags, and the tools')
def test_each_shared_piece_is_written_once(text, count):
    assert sum(src.count(text) for src in _sources().values()) == count


def test_the_tools_keep_to_public_names_of_each_other():
    src = _sources()
    assert sum(len(re.findall(r"^def _?num_labels\(", s, flags=re.M)) for s in src.values()) == 1
    assert not any(re.search(r"\._model\s*=", s) for s in src.values())                  # no model hidden on a parsed namespace
    tools = [f for f in src if f.startswith("compact_") and f not in ("compact_train.py", "compact_attribution.py")]
    short = r"\b(?:CT|PB|CC|OD|TL|RB|PX|PT)\._[a-z]"                                  # the tools' module aliases; CP._x is the long-standing base
    for f in tools:
        assert not re.search(short, src[f]), f
        for line in re.findall(r"^from \.compact_\w+ import .*$", src[f], flags=re.M):
            if f == "compact_robust.py" and line.startswith("from .compact_pixel import"):
                continue                                                     # (the class it subclasses, and that class's spec helpers)
            assert not re.search(r"[ ,]_\w+", " " + line.split(" import ", 1)[1]), (f, line)


def test_the_calibrator_does_not_import_the_probe():
    code = "import sys, uvc_amd.compact_calibrate; assert 'uvc_amd.compact_probe' not in sys.modules, 'compact_calibrate imported compact_probe'"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
