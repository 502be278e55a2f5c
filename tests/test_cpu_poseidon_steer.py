"""The steered Poseidon252 messages of tests/poseidon_steer.py, proven on the CPU (no GPU): every case puts the raw value it
claims into Hades round 0; the two limb models (felt_model.py for csrc/felt252.cuh, felt_coop_model.py for
csrc/felt252_coop.cuh) record every named carry, borrow and digit situation over the case set; and single-line faults planted
in the limb models change the state after round 0 of at least one case.  tests/test_gpu_poseidon_steer.py sends the same cases
to the device; its case list is held to this one by name."""
import collections
import inspect
import random

import pytest

import felt_coop_model as FC
import felt_model as F
import poseidon_model as M
import poseidon_steer as S
import test_cpu_felt_coop as TC

P, R = M.P, 2**256
MODELS = {"felt": F, "coop": FC}


# ---------------------------------------------------------------- forwards, on integers
def steered_absorb(case):
    """(state before the steered absorb, x, y) as integers"""
    if case.kind == "draw":
        return [0, 0, 2], case.digest, case.n_sent
    v = list(case.msg) + [1]
    if len(v) % 2:
        v.append(0)
    state = [0, 0, 0]
    for q in range(case.perm):
        state = M.hades([(state[0] + v[2 * q]) % P, (state[1] + v[2 * q + 1]) % P, state[2]])
    return state, v[2 * case.perm], v[2 * case.perm + 1]


def round0(state, x, y):
    """every raw value of round 0 a case may claim, and the state after the round"""
    rep = lambda v: v * R % P
    s = [(state[0] + x) % P, (state[1] + y) % P, state[2]]
    ark = M.ARK[0]
    pre = [(s[i] + ark[i]) % P for i in range(3)]
    a, b, c = (rep(pow(v, 3, P)) for v in pre)
    t = (a + b + c) % P
    raw = {"sum0": rep(s[0]) + rep(ark[0]), "sum1": rep(s[1]) + rep(ark[1]), "pre0": rep(pre[0]), "pre1": rep(pre[1]), "post0": a,
           "post1": b, "ab": a + b, "abc": (a + b) % P + c, "2A": 2 * a, "t-2B": t - 2 * b % P, "t-3c": t - 3 * c % P}
    return raw, [(t + 2 * a) % P, (t - 2 * b) % P, (t - 3 * c) % P]


def test_steering_identities():
    knobs = collections.Counter()
    for case in S.CASES:
        raw, _ = round0(*steered_absorb(case))
        assert case.claims or case.name.endswith("A0_Bmax"), case.name
        for key, want in case.claims.items():
            assert raw[key] == want, (case.name, key)
        if case.kind == "msg" and case.x_only:                 # as a one-element message: the appended 1 takes y's place
            raw1, _ = round0([0, 0, 0], case.msg[0], 1)
            for key, want in case.claims.items():
                if key in S.S0_KEYS or case.msg[1] == 1:
                    assert raw1[key] == want, (case.name, key, "k = 1")
        knobs[case.knob] += 1
    assert set(knobs) == {"pre-cube", "round-0 add", "post-cube", "later absorb", "channel draw"}
    assert {len(c.msg) for c in S.CASES if c.knob == "later absorb"} == {3, 4}
    assert {c.n_sent for c in S.CASES if c.kind == "draw"} == {0, 1, 2**32 - 2}


def test_cases_are_canonical_and_neighbours_carry_out():
    for case in S.CASES:
        assert all(0 <= v < P for v in (case.msg if case.kind == "msg" else [case.digest])), case.name
        if case.group_local:
            assert case.neighbour in S.BY_NAME, case.name
    # the neighbour of an all-borrow sub is the same sub without a borrow: its first resolve carries out of limb 7
    assert S.BY_NAME["post_t_is_2B-1"].neighbour == "post_t_is_2B+1" and S.BY_NAME["post_t_is_2B+1"].claims["t-2B"] == 1


# ---------------------------------------------------------------- the limb models against integers
def test_felt_model_against_integers():
    for a, b in TC._pairs():
        la, lb = F.limbs(a), F.limbs(b)
        assert F.value(F.mul(la, lb)) == a * b * F.R_INV % P
    rng = random.Random(8)
    vals = TC.EDGES + [rng.randrange(P) for _ in range(40)]
    for a in vals:
        for b in vals:
            assert F.value(F.add(F.limbs(a), F.limbs(b))) == (a + b) % P
            assert F.value(F.sub(F.limbs(a), F.limbs(b))) == (a - b) % P
    for t in (0, 1, P - 1, P, P + 1, 2 * P - 1, P - 1 + 2**192, 2**251, 2**252):
        assert F.value(F.reduce_once(F.limbs(t))) == t % P
    assert F.value(F.to_mont(F.limbs(P - 1))) == (P - 1) * R % P and F.value(F.from_mont(F.limbs(P - 1))) == (P - 1) * F.R_INV % P
    assert F.ARK == M.ARK == FC.ARK


@pytest.mark.parametrize("state", [[0, 0, 0], [P - 1, P - 2, P - 1], [2**251 - 1, 2**192 * 17, R % P]])
def test_felt_model_hades(state):
    assert F.hades(state) == M.hades(state)
    assert [v * R % P for v in F.hades(state, rounds=1)] == [v * R % P for v in FC.hades(state, rounds=1)] == round0(state, 0, 0)[1]


# ---------------------------------------------------------------- a case through a limb model
def _element(m, v, e):
    """element e of the padded message as the kernels' sponge forms it: to_mont of an input, the constant rep(1), or zero"""
    if e < len(v):
        return m.to_mont(m.limbs(v[e]))
    return list(m.ONE_L) if e == len(v) else m.limbs(0)


def run_case(m, case, msg=None, full=False):
    """the state after the steered absorb and round 0 as three Montgomery-form integers; full: the hash the entry returns.
    Everything before the steered absorb comes from the integer model, everything after it from the limb model m."""
    if msg is None and case.kind == "draw":
        s = [m.to_mont(m.limbs(case.digest)), m.to_mont(m.limbs(case.n_sent)), m.dbl(list(m.ONE_L))]
        if full:
            return m.value(m.from_mont(m.hades_mont(*s)[0]))
        return [m.value(x) for x in m.hades_mont(*s, rounds=1)]
    v = list(case.msg if msg is None else msg)
    perm = case.perm if msg is None else 0
    state, _, _ = steered_absorb(case) if msg is None else ([0, 0, 0], 0, 0)
    s = [m.limbs(x * R % P) for x in state]
    for q in range(perm, (len(v) + 2) // 2):
        s[0] = m.add(s[0], _element(m, v, 2 * q))
        s[1] = m.add(s[1], _element(m, v, 2 * q + 1))
        if not full:
            return [m.value(x) for x in m.hades_mont(*s, rounds=1)]
        s = list(m.hades_mont(*s))
    return m.value(m.from_mont(s[0]))


def want_case(case, msg=None, full=False):
    if full:
        return M.hash2(case.digest, case.n_sent) if msg is None and case.kind == "draw" else M.hash_many(case.msg if msg is None else msg)
    state, x, y = steered_absorb(case) if msg is None else ([0, 0, 0], msg[0], msg[1] if len(msg) > 1 else 1)
    return round0(state, x, y)[1]


@pytest.mark.parametrize("model", MODELS)
def test_limb_models_agree_with_integers_on_every_case(model):
    m = MODELS[model]
    for case in S.CASES:
        assert run_case(m, case) == want_case(case), case.name
    for name in ("sum_is_p", "post_ab_is_p_t_is_2B-1", "k4_post_t_is_3c-1", "draw1_post_t_is_2B-1"):
        assert run_case(m, S.BY_NAME[name], full=True) == want_case(S.BY_NAME[name], full=True), name


# ---------------------------------------------------------------- census
def census(m, monkeypatch, cases=S.CASES):
    events = collections.Counter()
    monkeypatch.setattr(m, "EVENTS", events)
    for case in cases:
        run_case(m, case)
    monkeypatch.setattr(m, "EVENTS", None)
    return events


@pytest.mark.parametrize("model", MODELS)
def test_census_every_named_event_is_reached(model, monkeypatch):
    m = MODELS[model]
    events = census(m, monkeypatch)
    print(f"\ncensus of {model} over {len(S.CASES)} cases:", *(f"  {n:24s} {events[n]}" for n in m.EVENT_NAMES + m.IMPOSSIBLE_EVENTS), sep="\n")
    assert [n for n in m.EVENT_NAMES if not events[n]] == []
    assert [n for n in m.IMPOSSIBLE_EVENTS if events[n]] == []
    assert set(events) <= set(m.EVENT_NAMES + m.IMPOSSIBLE_EVENTS)            # no event goes unnamed


# ---------------------------------------------------------------- mutants
# (name, model, function, the line as it stands, the line as broken).  Not in the list: faults that only get the choice between
# t and t - p (or d and d + p) wrong, such as reduce_once with > for >=, or a carry out of limb 7 that ignores a propagating
# lane 7.  They leave a value that is off by p, every operation that can follow works modulo p and reduces again, and only the
# reduction behind the last from_mont shows at an entry's output: round 0 cannot steer that one, so no case here kills them.
MUTANTS = [
    ("add: carry into limb 7 dropped", "felt", "add", "addc(a[k], b[k], c)", "addc(a[k], b[k], c if k < 7 else 0)"),
    ("sub: add-back without the ripple", "felt", "sub", "addc(d[k], P_L[k] & m, c)", "addc(d[k], P_L[k] & m, 0)"),
    ("mul: cc always 1", "felt", "mul", "cc = 1 if t[0] != 0 else 0", "cc = 1"),
    ("mul: r6's carry dropped", "felt", "mul", "r7 = (m << 27) + t[7] + (r6 >> 32)", "r7 = (m << 27) + t[7]"),
    ("subc: borrow-in on equal words lost", "felt", "subc", "1 if d < 0 else 0", "1 if a < b else 0"),
    ("addc: carry-in onto an all-ones sum lost", "felt", "addc", "return s & M32, s >> 32", "return s & M32, (a + b) >> 32"),
    ("resolve: no propagate mask", "coop", "resolve_wave", "a, b = (G | Pm) & LOW7, G & LOW7", "a, b = G & LOW7, G & LOW7"),
    ("resolve: no kLow7 masking", "coop", "resolve_wave", "a, b = (G | Pm) & LOW7, G & LOW7", "a, b = G | Pm, G"),
    ("mul: carries of the final L + from_lower(H) dropped", "coop", "mul", "t, top = resolve(last)", "t, top = [x & M32 for x in last], 0"),
    ("sub: add-back without carries", "coop", "sub", "r, _ = resolve([d[j] + (0 if no_borrow else P_L[j]) for j in range(8)], others)",
     "r = [(d[j] + (0 if no_borrow else P_L[j])) & M32 for j in range(8)]"),
    ("mul: H cut to 27 bits", "coop", "mul", "[x >> 32 for x in s]", "[(x >> 32) & (2**27 - 1) for x in s]"),
    ("mul: (m != 0) carry omitted", "coop", "mul", "(1 if j == 0 and m else 0)", "0"),
    ("mul: (m != 0) carry always taken", "coop", "mul", "(1 if j == 0 and m else 0)", "(1 if j == 0 else 0)"),
]


def plant(monkeypatch, mutant):
    """break one line of one function of a limb model, and silence the model's own checks so the wrong value comes out"""
    _, model, func, old, new = mutant
    m = MODELS[model]
    src = inspect.getsource(getattr(m, func))
    assert src.count(old) == 1, (func, old)
    scope = {}
    exec(compile(src.replace(old, new), m.__file__, "exec"), m.__dict__, scope)
    monkeypatch.setattr(m, func, scope[func])
    monkeypatch.setattr(m, "check", lambda *a: None)
    return m


def killers(m, cases, msgs=None):
    """names of the cases (or indices of the plain messages) whose state after absorb + round 0 the planted fault changes as
    field elements: a fault that only leaves p where 0 is due does not count, since nothing downstream can tell the two apart"""
    differs = lambda got, want: [v % P for v in got] != want
    if msgs is not None:
        return [i for i, msg in enumerate(msgs) if differs(run_case(m, None, msg=msg), want_case(None, msg=msg))]
    return [c.name for c in cases if differs(run_case(m, c), want_case(c))]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[x[0] for x in MUTANTS])
def test_mutant_is_killed_by_the_case_set(mutant, monkeypatch):
    m = plant(monkeypatch, mutant)
    dead = killers(m, S.CASES)
    print(f"\n{mutant[0]}: killed by {len(dead)} cases, first {dead[:3]}")
    assert dead, mutant[0]
    case = S.BY_NAME[dead[0]]
    assert run_case(m, case, full=True) != want_case(case, full=True), (mutant[0], case.name)      # ... and the hash differs too


def existing_messages():
    """the messages the device saw before: test_gpu_poseidon.py::test_hash_many_matches_model at k = 2, restated (the list is
    built inside that test), and every ordered EDGE pair of test_gpu_poseidon_coop.py"""
    import numpy as np
    import test_gpu_poseidon as G
    import test_gpu_poseidon_coop as GC
    rng = np.random.default_rng(100 + 2)
    many = [[G.EDGE[(i * 7 + j) % len(G.EDGE)] if (i + j) % 3 == 0 else int.from_bytes(rng.bytes(32), "little") % P for j in range(2)]
            for i in range(96)]
    return {"hash_many k=2": many, "coop EDGE pairs": [[a, b] for a in GC.EDGE for b in GC.EDGE]}


def test_mutants_on_the_existing_messages(monkeypatch):
    """Recorded, not asserted: which planted faults the earlier device inputs would have let through (same prefix)."""
    lists = existing_messages()
    print("\nmutant | killed by the steered cases | " + " | ".join(f"killed by {k} ({len(v)})" for k, v in lists.items()))
    for mutant in MUTANTS:
        with monkeypatch.context() as mp:
            m = plant(mp, mutant)
            row = [len(killers(m, S.CASES))] + [len(killers(m, None, msgs)) for msgs in lists.values()]
        print(f"{mutant[1]} {mutant[0]} | " + " | ".join(f"{n}" if n else "SURVIVES" for n in row))
    for model, m in MODELS.items():                                           # the census of the same messages, for the record
        for k, msgs in lists.items():
            ev = collections.Counter()
            monkeypatch.setattr(m, "EVENTS", ev)
            for msg in msgs:
                run_case(m, None, msg=msg)
            monkeypatch.setattr(m, "EVENTS", None)
            print(f"{model} events never reached by {k}: {[n for n in m.EVENT_NAMES if not ev[n]]}")


# ---------------------------------------------------------------- nothing is dropped on the way to the device
def test_gpu_file_runs_exactly_these_cases():
    import test_gpu_poseidon_steer as GS
    assert GS.CASE_NAMES == [c.name for c in S.CASES]
    assert len(set(GS.CASE_NAMES)) == len(GS.CASE_NAMES)
