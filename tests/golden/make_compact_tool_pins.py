#!/usr/bin/env python3
"""Record what the compact tools show to their callers into tests/golden/compact_tool_pins.json: the complete argparse surface of every
parser and subparser of ``compact_transfer``, ``compact_probe``, ``compact_calibrate``, ``compact_ood``, ``compact_robust``,
``compact_pixel`` and ``compact_perturb`` and of ``compact predict`` / ``explain`` / ``attribute`` (``make_driver_flag_pins.surface``'s
fields plus the bounds a type such as ``_int_in`` closes over), and, for fixed small CPU tensors, the keys, nested ``meta``, dtypes and
shapes of the four bank dicts.  Pure host code: no GPU, no library.  Run it at the commit whose tools are to be pinned -- BEFORE their
shared parts are merged; tests/test_compact_tool_pins_cpu.py compares a later tree against the file.

    python tests/golden/make_compact_tool_pins.py
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_driver_flag_pins import surface as driver_surface      # noqa: E402

TOOLS = ("compact_transfer", "compact_probe", "compact_calibrate", "compact_ood", "compact_robust", "compact_pixel", "compact_perturb")
META = dict(img_size=64, dataset="cifar10", split="test", interpolation="bicubic", crop_pct=0.9, precision="fp32", not_a_meta_key=1)


def surface(parser):
    """``make_driver_flag_pins.surface`` plus ``type_args``: the values a type made by a factory (``_int_in(lo, hi, what)``) closes over."""
    out = driver_surface(parser)
    for rec, a in zip(out, parser._actions):
        cells = getattr(a.type, "__closure__", None) or ()
        rec["type_args"] = [repr(c.cell_contents) for c in cells]
    return out


def _with_subparsers(name, parser):
    yield name, parser
    for a in parser._actions:
        if isinstance(a, argparse._SubParsersAction):
            for sub, q in a.choices.items():
                yield f"{name} {sub}", q


def parsers():
    """name -> parser: every tool's parser, ``"<tool> <command>"`` for its subparsers, and ``compact``'s three image-file commands."""
    import importlib
    from uvc_amd import compact
    out = {}
    for tool in TOOLS:
        out.update(_with_subparsers(tool, importlib.import_module("uvc_amd." + tool).build_parser()))
    sub = compact._parser()._subparsers._group_actions[0].choices
    out.update({"compact " + n: sub[n] for n in ("predict", "explain", "attribute")})
    return out


def _describe(v):
    import torch
    if torch.is_tensor(v):
        return dict(tensor=str(v.dtype), shape=list(v.shape), device=str(v.device), contiguous=v.is_contiguous())
    if isinstance(v, dict):
        return {k: _describe(v[k]) for k in sorted(v)}
    return dict(type=type(v).__name__, value=v)


def banks():
    """name -> the description of a bank dict made from fixed tensors: 5 rows, embed_dim 8, a 16-wide head over 10 classes."""
    import torch
    from uvc_amd import compact_calibrate as CC
    from uvc_amd import compact_ood as OD
    from uvc_amd import compact_probe as PB
    from uvc_amd import compact_transfer as CT
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(8, 5, generator=g, dtype=torch.float64).t()              # (neither float32 nor contiguous: the makers see to both)
    logits = torch.randn(5, 16, generator=g).to(torch.bfloat16)
    labels = torch.tensor([3, 1, 4, 1, 5], dtype=torch.int32)
    if hasattr(PB, "make_raw_bank"):
        raw = PB.make_raw_bank(feats, labels, 10, **META)
    else:                                            # (compact_probe.embed's own lines at the commit the pins were recorded at)
        raw = CT.make_bank(feats, labels, 10, **META)
        raw["normalized"] = False
    return {"transfer": _describe(CT.make_bank(feats, labels, 10, **META)), "probe_raw": _describe(raw),
            "logits": _describe(CC.make_logits_bank(logits, labels, 10, **META)),
            "ood": _describe(OD.make_ood_bank(feats, logits, labels, 10, **META))}


def main():
    pins = dict(parsers={name: surface(p) for name, p in parsers().items()}, banks=banks())
    with open(os.path.join(HERE, "compact_tool_pins.json"), "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in pins["parsers"].items()}, sorted(pins["banks"]))


if __name__ == "__main__":
    main()
