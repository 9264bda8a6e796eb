"""The planner's plans, pinned without a GPU: tools/plan_sweep.py --small plans the eight synthetic models of
tests/test_planner_sanitizers.py under the defaults, every planner switch one at a time, the six rule sets of that test and six opt-in
combinations, and this test compares the table it prints -- model, setting, bytes and SHA-256 of the plan's digest text
(tools/plan_digest.cpp), the constants' fnv= values left out of the hash because their bytes come from numpy and libm -- with
tests/golden/plan_sweep_small.txt.

A change to the planner's host code that is NOT meant to move a plan (a refactor) must leave the table as it is.  A change that IS meant to
move plans regenerates the table in the same commit:
    python tools/plan_sweep.py --small --strip-fnv > tests/golden/plan_sweep_small.txt
and its description says which rows moved and why.  (To compare two commits in full, constants included, run the script with
--full-text DIR on a checkout of each and diff the directories.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_plan_sweep_matches_the_table():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "plan_sweep.py"), "--small", "--strip-fnv"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "plan_sweep_small.txt")).read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    moved = [(w, g) for w, g in zip(want, got) if w != g]
    assert not moved, f"{len(moved)} of {len(want)} plans moved; the first (table, this tree):\n" + "\n".join(moved[0])
    # a table in which the fusion never fires pins nothing about it: 'stem:' and 'mbconv:' launches differ in count between these settings
    rows = {tuple(line.split()[:2]): line.split()[3] for line in got}
    assert rows[("v24", "defaults")] != rows[("v24", "BN_MBFUSE=0")] != rows[("v24", "BN_STEMFUSE=0")] != rows[("v24", "defaults")]
