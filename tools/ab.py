#!/usr/bin/env python3
"""A/B driver (GPU box): bench.py --full on N variants, run ALTERNATING, best / median and phase times per variant.

usage: tools/ab.py [--repeats 3] [--timeout 900] [--bench "<bench.py arguments>"] VARIANT [VARIANT ...]

A VARIANT is one quoted string of space-separated items ("-" = the default library, no settings):
  VAR=VALUE        an environment setting for the run (the runtime knobs of rzk_ctx_create, RZK_BENCH_DIAG=1, ...)
  lib=PATH         a prebuilt library (passed on as RZK_LIB)
  NAME:DEF=V,...   a library built with -DDEF=V ... (tools/ab_build.py; "NAME:" = no defines), built before the first run
e.g.  tools/ab.py - "RZK_SHIFT=0"        tools/ab.py --bench "--workload sum --shape 4,9,4" - "w2:RZK_ROW_MIN_WAVES=2"

Every bench.py child runs under its own time limit; the first child that fails or times out ends the whole run, and
nothing is started after it (no retries)."""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_build import build_variant  # noqa: E402


def environment(variant):
    env = {}
    for item in variant.split():
        if item == "-":
            continue
        if item.startswith("lib="):
            env["RZK_LIB"] = os.path.abspath(item[4:])
        elif ":" in item.split("=")[0]:
            env["RZK_LIB"] = build_variant(item)
        else:
            key, _, value = item.partition("=")
            env[key] = value
    return env


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per bench.py run")
    ap.add_argument("--bench", default="", help="arguments handed to bench.py")
    ap.add_argument("variants", nargs="+")
    args = ap.parse_args()
    envs = [environment(v) for v in args.variants]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline"] + shlex.split(args.bench)
    runs = [[] for _ in args.variants]
    for rep in range(args.repeats):
        for i, variant in enumerate(args.variants):
            # `timeout` ends the child's whole process group (bench.py may have started ranks of its own)
            p = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + cmd, env={**os.environ, **envs[i]}, cwd=ROOT,
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                why = f"ran longer than {args.timeout} s" if p.returncode in (124, 137) else f"exited with {p.returncode}"
                sys.exit(f"{variant!r}: bench.py {why}; stopping")
            lines = [line for line in p.stdout.splitlines() if line.startswith("{")]
            if not lines:
                sys.exit(f"{variant!r}: bench.py printed no JSON result line; stopping")
            j = json.loads(lines[-1])
            runs[i].append(j)
            print(f"run {rep + 1} {variant:30s} {j['value']:14.0f} /s", flush=True)
    for variant, js in zip(args.variants, runs):
        vals = [j["value"] for j in js]
        phases = {k: round(v, 1) for k, v in js[-1].get("roofline", {}).get("phase_us", {}).items()}
        print(f"{variant:30s} best {max(vals) / 1e6:8.3f} M  median {statistics.median(vals) / 1e6:8.3f} M  phases {phases}")


if __name__ == "__main__":
    main()
