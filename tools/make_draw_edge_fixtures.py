#!/usr/bin/env python3
"""Searches the channel states of tests/golden/blake2s_draw_edges.json (tests/draw_edges.py lists the cases).  NOT run by the suite:
a case costs 2^28 .. 2^30 trials of 1 to 20 hashes, seconds to minutes on 8 cores.

    python tools/make_draw_edge_fixtures.py [--redo] [--bound N] [case name or prefix ...]

Builds tools/draw_edge_search.c into a temporary directory, runs it once per case that the file does not hold yet (--redo: again
for the named ones), checks the reported digest on the hashlib model and rewrites the file after every case."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import draw_edges as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--redo", action="store_true")
    ap.add_argument("--bound", type=int, default=1 << 36)
    ap.add_argument("names", nargs="*")
    opt = ap.parse_args()
    doc = {"tag": "0xD4A3ED6E", "cases": {}}
    if os.path.exists(D.FIXTURE_PATH):
        with open(D.FIXTURE_PATH) as f:
            doc = json.load(f)
    with tempfile.TemporaryDirectory() as tmp:
        tool = os.path.join(tmp, "draw_edge_search")
        subprocess.check_call(["cc", "-O3", "-flto", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-o", tool,
                               os.path.join(ROOT, "tools", "draw_edge_search.c"), os.path.join(ROOT, "oracle", "tstwo_oracle.c")])
        for case in D.CASES:
            if opt.names and not any(case.name.startswith(n) for n in opt.names):
                continue
            if case.name in doc["cases"] and not (opt.redo and opt.names):
                continue
            args = [tool] + D.search_arguments(case, tmp) + ["--salt", str(D.salt(case)), "--bound", str(opt.bound)]
            t0 = time.time()
            rep = json.loads(subprocess.check_output(args))
            seconds = round(time.time() - t0, 1)
            if not rep["found"]:
                print(f"{case.name}: nothing within {opt.bound} trials ({seconds} s)")
                continue
            state = rep["digest"] + [D.N_CHALLENGES, case.n_sent]
            ch, _ = D.run_model(case, state)
            digest, n_sent, hashes = ch.draws[case.target]
            w = D.hash_words(digest, n_sent)
            assert D.condition_word(case.cond, w) == rep["word"] and f"0x{w[rep['word']]:08X}" == rep["value"], (case.name, rep)
            assert hashes == 1 + D.CONDITIONS[case.cond][2], (case.name, hashes)
            doc["cases"][case.name] = {"state": state, "draw": case.target, "cond": {"word": rep["word"], "value": rep["value"]},
                                       "search": {"cond": case.cond, "salt": D.salt(case), "lane": rep["lane"], "counter": rep["counter"],
                                                  "trials": rep["trials"], "seconds": seconds}}
            print(f"{case.name}: word {rep['word']} = {rep['value']} after {rep['trials']} trials, {seconds} s", flush=True)
            doc["cases"] = {c.name: doc["cases"][c.name] for c in D.CASES if c.name in doc["cases"]}
            with open(D.FIXTURE_PATH + ".tmp", "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
            os.replace(D.FIXTURE_PATH + ".tmp", D.FIXTURE_PATH)


if __name__ == "__main__":
    main()
