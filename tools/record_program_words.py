#!/usr/bin/env python3
"""Records the program words compile_program gives for three evals into tests/golden/air_program_words.json.

tests/test_cpu_interaction_trace.py compares the words of the current compiler with this file, so that a change to the compiler's
shared parts (canonicalisation, ordering, register allocation) that moves a single word of an existing program fails a test.
Run it on the commit whose words are the reference, not on the commit under test:

    python tools/record_program_words.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tstwo_amd import constraint_framework as F  # noqa: E402
from tstwo_amd.fields import QM31  # noqa: E402
from tstwo_amd.logup import LookupElements  # noqa: E402

LOG = 5
ELEMENTS = LookupElements(QM31.from_u32_unchecked(3, 4, 5, 6), QM31.from_u32_unchecked(7, 8, 9, 10), 2)
CLAIMED = QM31.from_u32_unchecked(11, 12, 13, 14)
# name -> (eval, claimed sum or None, preprocessed columns): what FrameworkComponent hands to ProgramEvaluator
CASES = {
    "wide_fibonacci_8": (F.WideFibonacciEval(LOG, 8), None, 0),
    "fibonacci_rows": (F.FibonacciRowsEval(LOG, 3, 4), None, 1),
    "permutation": (F.PermutationEval(LOG, ELEMENTS), CLAIMED, 0),
}


def program(eval_, claimed, n_pre):
    pe = F.ProgramEvaluator(claimed, eval_.log_size())
    eval_.evaluate(pe)
    pe.check_finished()
    return pe.compile(pe.n_main, n_pre)


def record():
    out = {}
    for name, (eval_, claimed, n_pre) in CASES.items():
        p = program(eval_, claimed, n_pre)
        out[name] = {"words": p.words, "n_regs": p.n_regs, "n_constraints": p.n_constraints, "n_loads": p.n_loads}
    return out


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "air_program_words.json")
    with open(path, "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
    print(path, {k: len(v["words"]) // 2 for k, v in record().items()})
