#!/usr/bin/env python3
"""Per-kernel table of `rocprofv3 --pmc` counter collections (no GPU needed).

Reads every ``*counter_collection.csv`` below the given directories and prints,
per kernel whose name contains ``--match`` and per counter, the number of
launches and the median value per launch - the form of the tables in
``profiles/twostep_lean/NOTES.md``. Counters of one table come from runs of
their own (a few counters per run, never with tracing).

Usage: python benchmarks/pmc_table.py DIR [DIR ...] [--match twostep]
"""
import argparse
import csv
import statistics
from collections import defaultdict
from pathlib import Path

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("dirs", nargs="+")
ap.add_argument("--match", default="twostep")
a = ap.parse_args()
vals = defaultdict(list)
for d in a.dirs:
    for f in sorted(Path(d).rglob("*counter_collection.csv")):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if a.match in r["Kernel_Name"]:
                    name = r["Kernel_Name"].replace("void igg::(anonymous namespace)::", "").split("(")[0]
                    vals[(name, r["Counter_Name"])].append(float(r["Counter_Value"]))
print("| kernel | counter | launches | median per launch |")
print("|---|---|---|---|")
for (k, c), v in sorted(vals.items()):
    print(f"| `{k}` | {c} | {len(v)} | {statistics.median(v):.0f} |")
