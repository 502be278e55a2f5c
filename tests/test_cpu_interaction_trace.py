"""The interaction trace derived from `evaluate`, on the host (no GPU): what RelationEvaluator records, the columns programs
compile_columns emits run through the integer model (tests/columns_model.py) against the numpy twins of the evals
(tests/interaction_evals.py), which expressions become program outputs, the words of compile_program against the fixture recorded
from the commit before compile_columns existed (tools/record_program_words.py), and the ValueErrors of the driver's plan."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, P

import columns_model as CM
import interaction_evals as E
from tstwo_amd import constraint_framework as F
from tstwo_amd import logup as LG
from tstwo_amd.air import ORIGINAL_TRACE_IDX
from tstwo_amd.fields import M31, QM31
from tstwo_amd.logup import RelationEntry

LE = E.elements()
LOGS = [1, 2, 3, 4, 6]


def rand_cols(log, k, seed):
    rng = np.random.default_rng(seed + 31 * log)
    return [rng.integers(0, P, size=1 << log, dtype=np.uint64) for _ in range(k)]


def is_load(e, column, offset=0):
    return isinstance(e, F.Expr) and e.op == "load" and e.args == (column, offset)


# ------------------------------------------------------------------ RelationEvaluator
def test_relation_evaluator_records_the_existing_examples():
    ev = F.relation_entries(F.PermutationEval(5, LE))
    assert ev.batching == [0, 0] and [m for _, m, _ in ev.entries] == [1, -1]
    assert all(rel is LE for rel, _, _ in ev.entries)
    assert is_load(ev.entries[0][2][0], ("main", 0)) and is_load(ev.entries[1][2][0], ("main", 1))
    assert ev.n_main == 2 and ev.n_interaction == 4 and ev.interaction_offsets == [[-1, 0]] * 4 and ev.constraints == []
    ev = F.relation_entries(F.RangeCheckTableEval(5, LE))
    (rel, mult, values), = ev.entries
    assert ev.batching == [0] and mult.op == "neg" and is_load(mult.args[0], ("main", 0)) and is_load(values[0], ("pre", 0))
    assert ev.pre_used == {0}
    ev = F.relation_entries(F.RangeCheckValuesEval(5, LE))
    assert ev.batching == [0, 0] and [m for _, m, _ in ev.entries] == [1, 1]


def test_relation_evaluator_records_the_state_machine_and_the_general_eval():
    ev = F.relation_entries(F.StateMachineEval(4, LE))
    assert ev.batching == [0, 0] and [m for _, m, _ in ev.entries] == [1, -1]
    x1, y = ev.entries[1][2]
    assert x1.op == "add" and is_load(x1.args[0], ("main", 0)) and x1.args[1].op == "const" and x1.args[1].args == 1
    assert is_load(y, ("main", 1))
    for batching, n_inter in (([0, 0], 4), ([0, 1], 8)):
        ev = F.relation_entries(E.GeneralEval(4, LE, batching))
        assert ev.batching == batching and ev.n_interaction == n_inter and ev.n_main == 4 and ev.pre_used == {0}
        assert ev.main_offsets == [[0], [0], [-1, 2], [0]]
        (_, m0, v0), (_, m1, v1) = ev.entries
        assert m0.op == "mul" and is_load(m0.args[0], ("main", 3)) and is_load(m0.args[1], ("pre", 0))
        assert v0[0].op == "sub" and is_load(v0[0].args[1], ("main", 2), -1) and v0[1].op == "sqr" and v0[2] == 7
        assert m1.op == "neg" and is_load(v1[0], ("main", 2), 2)
        # the last batch's column is read at [-1, 0], the others at [0]: the masks the prover's evaluators hand out
        assert ev.interaction_offsets[-4:] == [[-1, 0]] * 4 and ev.interaction_offsets[:-4] == [[0]] * (n_inter - 4)
    inf = F.info(E.GeneralEval(4, LE, [0, 1]))
    assert inf.mask_offsets()[2] == ev.interaction_offsets and inf.n_main == ev.n_main


def test_evaluate_without_relation_entries_is_refused():
    with pytest.raises(ValueError, match="no relation entries"):
        F.relation_entries(F.WideFibonacciEval(4, 8))
    with pytest.raises(ValueError, match="no relation entries"):
        LG.plan_interaction_trace(F.FibonacciRowsEval(4))


# ------------------------------------------------------------------ the programs against the twins
def plan_values(eval_, main, pre, log):
    """What the plan makes of every entry, as numpy: [(multiplicity, [values])], with the outputs of the compiled columns
    program from the integer model."""
    plan = LG.plan_interaction_trace(eval_)
    assert plan.n_main == len(main) and plan.n_pre == len(pre)
    outs = []
    if plan.exprs:
        program = F.compile_columns(plan.exprs, len(main), len(pre))
        assert program.n_out == len(plan.exprs) and program.n_regs <= F.MAX_REGS
        outs = CM.run_columns(program.words, main + pre, log, len(plan.exprs))

    def resolve(r):
        kind, x = r
        if kind == "const":
            return x.value if isinstance(x, M31) else x
        return outs[x] if kind == "out" else (main if x[0] == "main" else pre)[x[1]]
    entries = [(resolve(num), [resolve(r) for r in refs]) for batch in plan.batches for _, num, refs in batch]
    return plan, entries


def same_entries(got, want):
    assert len(got) == len(want)
    for (gm, gv), (wm, wv) in zip(got, want):
        assert np.array_equal(gm, wm) and len(gv) == len(wv)
        for g, w in zip(gv, wv):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("log", LOGS)
def test_columns_programs_equal_the_numpy_twins(log):
    """Offsets -1 and +2 of the general eval wrap around at log 1 (|2| >= 2^1).  The twins take their neighbours from the
    geometry; the same twins on a shift in coset order give the same columns."""
    nb = E.geometric_neighbours(log)
    main, pre = E.general_columns(log)
    for batching in ([0, 0], [0, 1]):
        _, got = plan_values(E.GeneralEval(log, LE, batching), main, pre, log)
        same_entries(got, E.general_twin(main, pre, nb))
    same_entries(E.general_twin(main, pre, E.coset_order_neighbours(log)), E.general_twin(main, pre, nb))
    xy = rand_cols(log, 2, 7)
    same_entries(plan_values(F.StateMachineEval(log, LE), xy, [], log)[1], E.state_machine_twin(xy, [], nb))
    same_entries(plan_values(F.PermutationEval(log, LE), xy, [], log)[1], E.permutation_twin(xy, [], nb))
    same_entries(plan_values(F.RangeCheckValuesEval(log, LE), xy, [], log)[1], E.values_twin(xy, [], nb))
    m, v = rand_cols(log, 2, 9)
    same_entries(plan_values(F.RangeCheckTableEval(log, LE), [m], [v], log)[1], E.table_twin([m], [v], nb))


class WrapEval:
    """One column read 5 and -7 rows away: beyond the whole trace at log 1 and 2."""

    def __init__(self, log):
        self.log = log

    def log_size(self):
        return self.log

    def evaluate(self, eval):
        far, back = eval.next_interaction_mask(ORIGINAL_TRACE_IDX, [5, -7])
        eval.add_to_relation(RelationEntry(LE, far, [back, far * back]))
        eval.finalize_logup()


@pytest.mark.parametrize("log", LOGS)
def test_offsets_beyond_the_trace_wrap_around(log):
    c, = rand_cols(log, 1, 11)
    for nb in (E.geometric_neighbours(log), E.coset_order_neighbours(log)):
        far, back = c[nb(5)], c[nb(-7)]
        same_entries(plan_values(WrapEval(log), [c], [], log)[1], [(far, [back, far * back % P])])
    n = 1 << log
    assert np.array_equal(E.geometric_neighbours(log)(5), E.geometric_neighbours(log)(5 % n))


def test_state_machine_trace_holds_consecutive_states_in_coset_order():
    import logup_model as LM
    x, y = F.state_machine_trace(5, P - 3, 9)
    assert x.dtype == np.uint32 and np.array_equal(x[LM.positions(5)].astype(np.int64), (P - 3 + np.arange(32)) % P) and (y == 9).all()


# ------------------------------------------------------------------ which expressions become outputs
def test_bare_loads_at_offset_zero_produce_no_program_output():
    assert LG.plan_interaction_trace(F.PermutationEval(4, LE)).exprs == []
    assert LG.plan_interaction_trace(F.RangeCheckValuesEval(4, LE)).exprs == []
    plan = LG.plan_interaction_trace(F.RangeCheckTableEval(4, LE))
    assert [e.op for e in plan.exprs] == ["neg"] and plan.batches[0][0][1] == ("out", 0) and plan.batches[0][0][2] == [("col", ("pre", 0))]
    plan = LG.plan_interaction_trace(F.StateMachineEval(4, LE))
    (_, n0, r0), (_, n1, r1) = plan.batches[0]
    assert [e.op for e in plan.exprs] == ["add"]
    assert n0 == ("const", M31(1)) and r0 == [("col", ("main", 0)), ("col", ("main", 1))]
    assert n1 == ("const", M31(P - 1)) and r1 == [("out", 0), ("col", ("main", 1))]
    # a load at another row is an output, a constant value is a constant
    plan = LG.plan_interaction_trace(E.GeneralEval(4, LE))
    assert len(plan.exprs) == 5 and plan.batches[0][0][2][2] == ("const", M31(7)) and plan.batches[0][1][2] == [("out", 4)]


class SharedEval:
    def log_size(self):
        return 3

    def evaluate(self, eval):
        x, y = eval.next_trace_mask(), eval.next_trace_mask()
        eval.add_to_relation(RelationEntry(LE, x * y + 1, [x + 1, y]))
        eval.add_to_relation(RelationEntry(LE, 2, [x + 1, 1 + x, y * x + 1]))          # x + 1 again; 1 + x and y x + 1 are other trees
        eval.finalize_logup_in_pairs()


def test_equal_expressions_share_an_output():
    plan = LG.plan_interaction_trace(SharedEval())
    (_, n0, r0), (_, n1, r1) = plan.batches[0]
    assert len(plan.exprs) == 4
    assert n0 == ("out", 0) and r0 == [("out", 1), ("col", ("main", 1))]
    assert n1 == ("const", M31(2)) and r1 == [("out", 1), ("out", 2), ("out", 3)]
    x, y = rand_cols(3, 2, 5)
    _, got = plan_values(SharedEval(), [x, y], [], 3)
    same_entries(got, [((x * y + 1) % P, [(x + 1) % P, y]), (2, [(x + 1) % P, (x + 1) % P, (x * y + 1) % P])])


class ManyEval:
    """k entries with the distinct values x + 1 .. x + k, one batch each."""

    def __init__(self, k):
        self.k = k

    def log_size(self):
        return 3

    def evaluate(self, eval):
        x = eval.next_trace_mask()
        for i in range(self.k):
            eval.add_to_relation(RelationEntry(LE, 1, [x + (i + 1)]))
        eval.finalize_logup()


def test_more_than_64_expressions_do_not_fit_one_program():
    plan = LG.plan_interaction_trace(ManyEval(70))
    assert len(plan.exprs) == 70 and len(plan.batches) == 70
    assert F.compile_columns(plan.exprs[:F.MAX_OUT], 1).n_out == 64
    with pytest.raises(ValueError, match="1 to 64 outputs"):
        F.compile_columns(plan.exprs, 1)
    with pytest.raises(ValueError, match="1 to 64 outputs"):
        F.compile_columns([], 1)


# ------------------------------------------------------------------ compile_program is what it was
def _program(eval_, claimed, n_pre):
    pe = F.ProgramEvaluator(claimed, eval_.log_size())
    eval_.evaluate(pe)
    pe.check_finished()
    return pe.compile(pe.n_main, n_pre)


def test_compile_program_words_are_unchanged():
    """The fixture holds the words of the commit before compile_columns shared the compiler (tools/record_program_words.py)."""
    with open(os.path.join(GOLDEN, "air_program_words.json")) as f:
        want = json.load(f)
    le = LG.LookupElements(QM31.from_u32_unchecked(3, 4, 5, 6), QM31.from_u32_unchecked(7, 8, 9, 10), 2)
    cases = {"wide_fibonacci_8": (F.WideFibonacciEval(5, 8), None, 0), "fibonacci_rows": (F.FibonacciRowsEval(5, 3, 4), None, 1),
             "permutation": (F.PermutationEval(5, le), QM31.from_u32_unchecked(11, 12, 13, 14), 0)}
    assert sorted(want) == sorted(cases)
    for name, (eval_, claimed, n_pre) in cases.items():
        p = _program(eval_, claimed, n_pre)
        assert p.words == want[name]["words"], name
        assert (p.n_regs, p.n_constraints, p.n_loads) == (want[name]["n_regs"], want[name]["n_constraints"], want[name]["n_loads"])
        assert not any(w & 0xff == F.OP_STORE for w in p.words[::2])


def test_compile_columns_is_compile_program_with_stores():
    """The same expressions through both compilers: the same words except that the k-th ACC is STORE k."""
    ev = F.ProgramEvaluator()
    F.FibonacciRowsEval(4).evaluate(ev)
    prog, cols = F.compile_program(ev.constraints, 2, 1), F.compile_columns(ev.constraints, 2, 1)
    want, k = CM.stores_for_accs(prog.words)
    assert cols.words == want and k == cols.n_out == 4 and cols.n_regs == prog.n_regs


# ------------------------------------------------------------------ the errors of the plan
class OneEntry:
    def __init__(self, entry, batching=None, size=3, repeat=1):
        self.entry, self.batching, self.size, self.repeat = entry, batching, size, repeat

    def log_size(self):
        return 3

    def evaluate(self, eval):
        le = E.elements(self.size)
        x, y = eval.next_trace_mask(), eval.next_trace_mask()
        for _ in range(self.repeat):
            mult, values = self.entry(x, y)
            eval.add_to_relation(RelationEntry(le, mult, values))
        eval.finalize_logup_batched(self.batching if self.batching is not None else range(self.repeat))


def test_plan_errors():
    plan = LG.plan_interaction_trace
    with pytest.raises(ValueError, match="1 to 16 column terms"):                         # no column among the values
        plan(OneEntry(lambda x, y: (x, [3, M31(4)])))
    with pytest.raises(ValueError, match="1 to 16 column terms"):
        plan(OneEntry(lambda x, y: (1, [F.Expr.const(5)])))
    with pytest.raises(ValueError, match="secure"):
        plan(OneEntry(lambda x, y: (QM31.from_u32_unchecked(1, 2, 3, 4), [x])))
    with pytest.raises(ValueError, match="secure"):
        plan(OneEntry(lambda x, y: (F.SecureExpr.lift(x) * QM31.from_u32_unchecked(1, 2, 3, 4), [x])))
    with pytest.raises(ValueError, match="secure"):
        plan(OneEntry(lambda x, y: (1, [F.SecureExpr.lift(x) * QM31.from_u32_unchecked(1, 2, 3, 4)])))
    with pytest.raises(ValueError, match="at most 8 fractions per column"):
        plan(OneEntry(lambda x, y: (1, [x]), batching=[0] * 9, repeat=9))
    plan(OneEntry(lambda x, y: (1, [x]), batching=[0] * 8, repeat=8))
    with pytest.raises(ValueError, match="1 to 16 column terms"):
        plan(OneEntry(lambda x, y: (1, [x + i for i in range(17)]), size=17))
    plan(OneEntry(lambda x, y: (1, [x + i for i in range(16)] + [5]), size=17))             # 16 columns and a constant
    with pytest.raises(ValueError, match="4 values for a relation of size 3"):
        plan(OneEntry(lambda x, y: (1, [x, y, x, y])))
    with pytest.raises(TypeError):
        plan(OneEntry(lambda x, y: (1.5, [x])))


def test_new_names_are_exported():
    import tstwo_amd as T
    assert T.derive_interaction_trace is LG.derive_interaction_trace is T.deriveInteractionTrace
    assert T.StateMachineEval is F.StateMachineEval and T.RelationEvaluator is F.RelationEvaluator
    assert T.compile_columns is F.compile_columns and T.evaluate_columns is F.evaluate_columns and T.state_machine_trace is F.state_machine_trace
    assert "tstwo_air_eval_columns" in T._lib.EXPORTS
