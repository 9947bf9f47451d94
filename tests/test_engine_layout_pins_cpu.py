"""CPU: the host-side queries of the two engines (include/uvc_vit.h) against the values recorded before their shared plumbing moved
into csrc/engine_host.h (tests/golden/engine_layout_pins.json, written by tests/golden/make_engine_layout_pins.py): parameter and
shadow layouts, workspace sizes, workspace offsets and frozen ranges are what they were.  The one exception is the compact eval
workspace, which lost the third residual-row buffer nothing read or wrote: it is the recorded size minus that buffer.  No GPU."""
import json
import os

import pytest

import make_engine_layout_pins as MP

with open(os.path.join(os.path.dirname(os.path.abspath(MP.__file__)), "engine_layout_pins.json")) as f:
    PINS = json.load(f)


@pytest.fixture(scope="module")
def lib():
    return MP.bind()


def test_every_case_is_recorded():
    assert sorted(PINS) == sorted(MP.CASES)


def test_the_cases_cover_what_training_refuses():
    assert PINS["d192_384px_bf16"]["compact_train_layout"] == dict(rc=3) and PINS["d192_384px_bf16"]["compact_train_workspace_bytes"] == [-1, -1]
    assert PINS["d128_mixed_bf16_f32resid"]["compact_train_layout"] == dict(rc=3)
    assert all(n > 0 for name in PINS for n in PINS[name]["compact_workspace_bytes"])
    assert all(n > 0 for n in PINS["d128_mixed_bf16"]["compact_train_workspace_bytes"] + PINS["d128_no_blocks"]["compact_train_workspace_bytes"])


def dropped_residual_buffer(case, B):
    """Bytes of one residual-stream buffer [B * N, D] in the workspace (256-byte aligned, as the carver hands them out)."""
    c = case["cfg"]
    N = (c["img_size"] // c["patch_size"]) ** 2 + c["ntok"]
    rsz = 2 if c["dtype"] == 1 and not c.get("resid_f32", 0) else 4
    return (B * N * c["embed_dim"] * rsz + 255) // 256 * 256


@pytest.mark.parametrize("name", sorted(MP.CASES))
def test_host_queries_answer_what_they_did(lib, name):
    got, want = MP.query(lib, MP.CASES[name]), PINS[name]
    assert sorted(got) == sorted(want)
    for key in want:
        if key != "compact_workspace_bytes":
            assert got[key] == want[key], key
    for B, g, w in zip(MP.BATCHES, got["compact_workspace_bytes"], want["compact_workspace_bytes"]):
        assert g == w - dropped_residual_buffer(MP.CASES[name], B) and g <= w, (B, g, w)
