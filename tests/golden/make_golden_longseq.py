#!/usr/bin/env python3
"""Generate the long-sequence golden fixtures (longseq_*.npz) from the REFERENCE's own modules, exactly as make_golden.py does for
the scenarios of scenarios.py: the scenarios are those of longseq_scenarios.py (registered into scenarios.py's tables in this process only), and each is run by
make_golden.run_scenario.  Runs only where the reference is available; the tests only read the .npz files.
Usage:  python tests/golden/make_golden_longseq.py [scenario ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import longseq_scenarios as LS  # noqa: E402
import make_golden  # noqa: E402

# the fixtures the tests pin against: fp32 Stage-1 steps at N = 577 (with and without patch gating mode 2) and N = 785
GOLDEN = ["longseq_p4_96_pruned", "longseq_p4_96_patch2", "longseq_p4_112_pruned"]

if __name__ == "__main__":
    LS.register()
    for n in sys.argv[1:] or GOLDEN:
        assert n in LS.LONG_SCENARIOS, n
        make_golden.run_scenario(n)
