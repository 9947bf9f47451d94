"""CPU: the drivers' command lines are what they were before their flag blocks were merged (uvc_amd/driver.py): every action of the
five parsers, in order, with its option strings, dest, type, default, choices, nargs, required and help, against
tests/golden/driver_flag_pins.json (recorded by tests/golden/make_driver_flag_pins.py before the merge).  And uvc_amd.data no longer
imports a driver."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARSERS = ["stage1", "stage2", "compact_export", "compact_eval", "compact_finetune"]


@pytest.fixture(scope="module")
def surfaces(request):
    sys.path.insert(0, GOLDEN)
    request.addfinalizer(lambda: sys.path.remove(GOLDEN))
    import make_driver_flag_pins as M
    saved = os.environ.get("LOCAL_RANK")
    try:
        now = {name: M.surface(p) for name, p in M.parsers().items()}       # (unsets LOCAL_RANK: --local_rank's default reads it)
    finally:
        if saved is not None:
            os.environ["LOCAL_RANK"] = saved
    with open(os.path.join(GOLDEN, "driver_flag_pins.json")) as f:
        return json.loads(json.dumps(now)), json.load(f)


def test_the_pins_cover_the_five_parsers(surfaces):
    now, pins = surfaces
    assert sorted(pins) == sorted(PARSERS) == sorted(now)


@pytest.mark.parametrize("name", PARSERS)
def test_parser_surface_is_the_pinned_one(surfaces, name):
    now, pins = surfaces
    assert [a["option_strings"] for a in now[name]] == [a["option_strings"] for a in pins[name]]
    for got, want in zip(now[name], pins[name]):
        assert got == want, want["option_strings"]


def test_data_module_does_not_import_a_driver():
    code = "import sys, uvc_amd.data; assert 'uvc_amd.cli' not in sys.modules, 'uvc_amd.data imported uvc_amd.cli'"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
