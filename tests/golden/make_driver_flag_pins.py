#!/usr/bin/env python3
"""Record the complete argparse surface of the drivers into tests/golden/driver_flag_pins.json: for each of the five parsers
(Stage 1, Stage 2, ``compact export`` / ``eval`` / ``finetune``) every action in order with its option strings, dest, type name,
default, choices, nargs, required and help.  Pure host code: no GPU, no library.  Run it at the commit whose flags are to be pinned --
BEFORE the flag blocks are restructured; tests/test_driver_flags_cpu.py compares a later tree against the file.

    python tests/golden/make_driver_flag_pins.py
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def surface(parser):
    """Every action of ``parser`` in order, as JSON-able values."""
    return [dict(option_strings=list(a.option_strings), dest=a.dest, type=None if a.type is None else a.type.__name__, default=a.default,
                 choices=None if a.choices is None else list(a.choices), nargs=a.nargs, required=bool(a.required), help=a.help)
            for a in parser._actions]


def parsers():
    """name -> parser.  --local_rank's default reads the environment: recorded with LOCAL_RANK unset."""
    os.environ.pop("LOCAL_RANK", None)
    from uvc_amd import cli, compact, post_train
    sub = compact._parser()._subparsers._group_actions[0].choices
    return {"stage1": cli.build_parser(), "stage2": post_train.add_stage2_flags(argparse.ArgumentParser()),
            "compact_export": sub["export"], "compact_eval": sub["eval"], "compact_finetune": sub["finetune"]}


def main():
    pins = {name: surface(p) for name, p in parsers().items()}
    with open(os.path.join(HERE, "driver_flag_pins.json"), "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in pins.items()})


if __name__ == "__main__":
    main()
