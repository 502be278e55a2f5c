"""What tests/sequence.py does without a GPU: the chained references against the oracle called directly, the generator's
determinism, and the failure report on a fabricated "device" image."""
import numpy as np
import pytest

from conftest import P, rand_column
from oracle import oracle as orc
import sequence as SQ


def test_chain_evaluate_commit_fold_equals_the_oracle_called_directly():
    """extend -> evaluate (in place) -> Merkle commit -> circle fold -> line fold, no host step between: Seq.expected() must give
    what the oracle gives when each step is fed the previous step's result by hand."""
    s = SQ.Seq()
    small = rand_column(1, 1 << 5)
    others = [rand_column(2 + i, 1 << 7) for i in range(3)]
    ext = SQ.poly_extend(s, s.inputs([small])[0], 5, 7)
    ev = SQ.cfft(s, "evaluate", [ext] + s.inputs(others), 7)
    layers = SQ.merkle_commit(s, ev, [7] * 4)
    line = SQ.fold_circle_into_line(s, "tw", [SQ.zero(s, 1 << 6) for _ in range(4)], ev, 7)
    out = SQ.fold_line(s, "tw", line, 6)
    state, writer = s.expected()

    half = SQ.half_odds(6)
    tw = orc.precompute_twiddles(half, 6)[0]
    padded = np.zeros(1 << 7, dtype=np.uint32)
    padded[:1 << 5] = small
    evs = [orc.cfft_evaluate(c, 7, half, tw, 6) for c in [padded] + others]
    olayers, _ = orc.merkle_commit(evs, [7] * 4)
    oline = orc.fold_circle_into_line([np.zeros(1 << 6, dtype=np.uint32)] * 4, evs, 7, half, SQ.ALPHA)
    oout = orc.fold_line(oline, 6, SQ._line_setup(6)[1], SQ.ALPHA)
    for k in range(4):
        assert (state[ev[k]] == evs[k]).all()
        assert (state[line[k]] == oline[k]).all()
        assert (state[out[k]] == oout[k]).all()
    assert state[layers].tobytes() == np.concatenate(olayers).tobytes()
    assert [s.ops[writer[ev[0]]].entry, s.ops[writer[line[0]]].entry] == ["tstwo_cfft_evaluate", "tstwo_fri_fold_circle_into_line_tw"]


def test_chain_field_ops_in_place_and_copies_equals_the_oracle_called_directly():
    s = SQ.Seq()
    a, b = rand_column(10, 1021, nonzero=True), rand_column(11, 1021)
    x4, y4 = [rand_column(20 + i, 128) for i in range(4)], [rand_column(30 + i, 128) for i in range(4)]
    na, nb = s.inputs([a, b])
    t = SQ.m31_op(s, "neg", SQ.m31_op(s, "mul", SQ.m31_op(s, "add", na, nb), na))
    q = SQ.qm31_mul(s, s.inputs(x4), s.inputs(y4))
    keep = [SQ.copy(s, c) for c in q]
    SQ.secure_accumulate(s, q, keep)                     # q += its own copy, in place
    inv = SQ.batch_inverse_async(s, [SQ.m31_op(s, "mul", na, na)])     # squares of nonzero words are nonzero
    state, _ = s.expected()
    assert (state[t] == orc.col_op("neg", orc.col_op("mul", orc.col_op("add", a, b), a))).all()
    prod = orc.qm31_col_mul(x4, y4)
    for k in range(4):
        assert (state[keep[k]] == prod[k]).all()
        assert (state[q[k]] == orc.col_op("add", prod[k], prod[k])).all()
    assert (orc.col_op("mul", state[inv[0]], orc.col_op("mul", a, a)) == 1).all()
    assert (state[na] == a).all() and (state[nb] == b).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_generator_is_deterministic_per_seed_and_defines_every_output(seed):
    s1, s2 = SQ.random_sequence(seed, n_ops=24), SQ.random_sequence(seed, n_ops=24)
    assert s1.signature() == s2.signature() and s1.sizes == s2.sizes
    assert (s1.image() == s2.image()).all()
    st1, w1 = s1.expected()
    st2, w2 = s2.expected()
    assert w1 == w2 and all((st1[n] == st2[n]).all() for n in st1)
    assert SQ.random_sequence(seed + 100, n_ops=24).signature() != s1.signature()
    assert len(s1.ops) >= 24
    for name in w1:                                       # no op leaves a word of an output it claims to the sentinel
        assert (st1[name] != SQ.SENTINEL).all(), (name, s1.ops[w1[name]].entry)
    users = [op.scratch for op in s1.ops if op.scratch]
    assert users[:6] == ["quotient blob", "air program", "logup descriptors", "gkr eq tables", "gkr ticket and slab", "quotient blob"]


def test_capturable_sequence_has_one_structure_for_every_data_seed():
    s1, s2 = SQ.capturable_sequence(0), SQ.capturable_sequence(1)
    assert s1.signature() == s2.signature() and s1.layout() == s2.layout()
    assert not (s1.image() == s2.image()).all()
    entries = {op.entry for op in s1.ops}
    assert {"tstwo_gkr_sum_poly_async", "tstwo_gkr_round", "tstwo_gkr_gen_eq_evals"} <= entries
    assert not entries & {"tstwo_upload", "tstwo_logup_column", "tstwo_air_eval_program", "tstwo_quotients_accumulate_async"}
    s1.expected()


def test_failure_report_names_the_op_the_output_and_the_differing_words():
    s = SQ.Seq()
    a, b = s.inputs([rand_column(1, 300), rand_column(2, 300)])
    t0 = SQ.m31_op(s, "add", a, b)             # op 0
    t1 = SQ.m31_op(s, "mul", t0, b)            # op 1
    t2 = SQ.copy(s, t1)                        # op 2
    state, _ = s.expected()
    start, total = s.layout()
    img = np.full(total // 4, SQ.SENTINEL, dtype=np.uint32)
    for n, w in state.items():
        img[start[n] // 4:start[n] // 4 + w.size] = w
    assert SQ.compare(s, img) == []
    bad = img.copy()                           # the "device" got words 7 and 250 of op 1's output wrong, and the copy carried them on
    for name in (t1, t2):
        bad[start[name] // 4 + 7] ^= 1
        bad[start[name] // 4 + 250] ^= 4
    msgs = SQ.compare(s, bad)
    assert len(msgs) == 2
    assert msgs[0].startswith(f"op #1 tstwo_m31_mul: output '{t1}': first differing word 7 ") and "last differing word 250" in msgs[0]
    assert msgs[1].startswith(f"op #2 tstwo_copy: output '{t2}'")
    assert "2 of 300 words differ" in msgs[0]
    bad = img.copy()
    bad[start[a] // 4 + 3] = 0                 # a stray store into an input
    assert SQ.compare(s, bad) == [m for m in SQ.compare(s, bad) if m.startswith(f"buffer '{a}' that no op writes was modified")]
    assert len(SQ.compare(s, bad)) == 1
