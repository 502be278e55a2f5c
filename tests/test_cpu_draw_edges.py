"""The steered channel states of tests/golden/blake2s_draw_edges.json, proven without a GPU: every fixture puts the word it claims
into the first hash of the draw it claims (hashlib, raw words); tstwo_amd/channel.py draws what the model draws from them; every
planted fault of tests/draw_edges.py is killed by every entry's case list; tests/test_gpu_draw_edges.py is held to the same lists by
name; and the search tool, built with AddressSanitizer and UBSan as a program of its own, re-finds every fixture at its recorded
counter and reports the same thing twice."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

import draw_edges as D

P = D.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = D.load_fixtures()
reduce_ = lambda x: x - P if x >= P else x      # noqa: E731


def raw_hash(digest, n_sent):
    return struct.unpack("<8I", hashlib.blake2s(digest + n_sent.to_bytes(4, "little") + bytes(28)).digest())


def steered_draw(case):
    """(digest, n_sent) on entry to the steered draw of a case, from the model's run of the whole entry"""
    ch, _ = D.run_model(case, FIX[case.name]["state"])
    digest, n_sent, hashes = ch.draws[case.target]
    return digest, n_sent, hashes


# ---------------------------------------------------------------- the fixtures
def test_the_file_holds_exactly_the_cases():
    assert list(FIX) == [c.name for c in D.CASES]
    assert os.path.getsize(D.FIXTURE_PATH) < 64 * 1024
    assert sorted(n for names in D.ENTRY_LISTS.values() for n in names) == sorted(FIX)
    import gkr_model as M
    assert (D.GP, D.GENERIC) == (M.GP, M.GENERIC)


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_fixture_on_raw_hash_words(name):
    case, fx = D.BY_NAME[name], FIX[name]
    assert fx["draw"] == case.target and fx["state"][9] == case.n_sent and fx["search"]["cond"] == case.cond
    assert fx["state"][0] == D.TAG and fx["state"][4] == D.salt(case) == fx["search"]["salt"]
    digest, s, hashes = steered_draw(case)
    w = raw_hash(digest, s)
    k, value = fx["cond"]["word"], int(fx["cond"]["value"], 16)
    words, values, rejected = D.CONDITIONS[case.cond]
    assert w[k] == value and k in words and value in values and D.condition_word(case.cond, list(w)) == k
    if case.cond.startswith("rej_hi"):
        assert all(x < 2 * P for x in w[:4])
    if rejected:
        assert any(x >= 2 * P for x in w)
        w2 = raw_hash(digest, s + 1)
        assert all(x < 2 * P for x in w2), "the redraw is accepted"
        want = (tuple(reduce_(x) for x in w2[:4]), s + 2, 2)
    else:
        assert all(x < 2 * P for x in w)
        want = (tuple(reduce_(x) for x in w[:4]), s + 1, 1)
        assert reduce_(w[k]) == {2 * P - 1: P - 1, P: 0}[value] and (k >= 4 or want[0][k] == reduce_(w[k]))
    assert D.draw(digest, s) == want and hashes == want[2]
    assert all(x < P for x in want[0])


def test_conditions_cover_the_issue_s_table():
    conds = {c.cond for c in D.CASES if c.entry == "draw"}
    assert conds == {"rej_lo_2P", "rej_lo_max", "rej_hi_2P", "rej_hi_max", "acc_lo_top", "acc_hi_top", "acc_P"}
    assert {c.n_sent for c in D.CASES if c.entry == "draw"} == {0, 5}
    for entry in ("draw", "mix"):
        assert [c.name.split("/", 1)[1] for c in D.CASES if c.entry == entry] == D.STANDALONE_CONDS


# ---------------------------------------------------------------- the host twin
STANDALONE = [c.name for c in D.CASES if c.entry in ("draw", "mix")]


def host_channel(state, ts_compat):
    from tstwo_amd.channel import Blake2sChannel
    ch = Blake2sChannel(ts_compat=ts_compat)
    ch._digest, ch.n_challenges, ch.n_sent = struct.pack("<8I", *state[:8]), state[8], state[9]
    return ch


@pytest.mark.parametrize("ts_compat", [False, True], ids=["rust", "ts_compat"])
@pytest.mark.parametrize("name", STANDALONE)
def test_host_channel_draws_what_the_model_draws(name, ts_compat):
    case, state = D.BY_NAME[name], FIX[name]["state"]
    model, felt = D.run_model(case, state)
    ch = host_channel(state, ts_compat)
    if case.entry == "mix":
        ch.mix_root(D.ROOT)
    assert ch.draw_felt().tup() == felt
    assert [*struct.unpack("<8I", ch.digest()), ch.n_challenges, ch.n_sent] == model.words()
    # draw_felts(2) takes both felts from the 8 words of ONE accepted hash: across the rejected one where there is one
    ch = host_channel(state, ts_compat)
    if case.entry == "mix":
        ch.mix_root(D.ROOT)
    digest, s, hashes = model.draws[0]
    w = raw_hash(digest, s + hashes - 1)
    assert all(x < 2 * P for x in w)
    assert [f.tup() for f in ch.draw_felts(2)] == [tuple(reduce_(x) for x in w[:4]), tuple(reduce_(x) for x in w[4:])]
    assert ch.n_sent == s + hashes and ch.digest() == digest


# ---------------------------------------------------------------- planted faults
def outcome(case, fault):
    ch, out = D.run_model(case, FIX[case.name]["state"], fault)
    return ch.words(), repr(out)


@pytest.mark.parametrize("entry", list(D.ENTRY_LISTS))
@pytest.mark.parametrize("fault", list(D.FAULTS))
def test_fault_is_killed_by_the_entry_s_list(fault, entry):
    """At least one case of the list gives an output or an end state that differs from the true model's: every fault, every list."""
    killers = [n for n in D.ENTRY_LISTS[entry] if outcome(D.BY_NAME[n], fault) != outcome(D.BY_NAME[n], None)]
    print(f"\n({fault}) {D.FAULTS[fault]} on {entry}: killed by {killers}")
    assert killers, (fault, entry)


# the fault that a case of each kind of condition must show on its own: a vacuous case fails here, without a GPU
FAULT_OF_VALUE = {2 * P: "a", 2 * P + 1: "a", 2 * P - 1: "d", P: "f"}


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_every_case_shows_a_fault_of_its_own(name):
    case = D.BY_NAME[name]
    fault = FAULT_OF_VALUE[int(FIX[name]["cond"]["value"], 16)]
    changed = [f for f in D.FAULTS if outcome(case, f) != outcome(case, None)]
    if name in D.UNOBSERVABLE:
        assert changed == [], "no output of the entry depends on this draw: draw_edges.UNOBSERVABLE says why"
    else:
        assert fault in changed, (name, changed)
        if D.CONDITIONS[case.cond][2]:
            assert {"a", "e", "g"} <= set(changed), (name, changed)       # every rejection shows the three retry faults


def test_unobservable_cases_are_few_and_named():
    assert list(D.UNOBSERVABLE) == ["prove/begin0"]
    assert len([n for n in D.ENTRY_LISTS["gkr prove_batch"] if n not in D.UNOBSERVABLE]) >= 4


def test_the_model_s_faults_are_single_and_silent_off_the_edges():
    """away from the edges (an ordinary state) no fault changes anything: the suite could not see them before"""
    for seed in range(8):
        digest = hashlib.blake2s(bytes([seed])).digest()
        for fault in D.FAULTS:
            assert D.draw(digest, seed, fault) == D.draw(digest, seed)


# ---------------------------------------------------------------- nothing is dropped on the way to the device
def test_gpu_file_runs_exactly_these_cases():
    """the parametrisation pytest collects from the GPU file, read from the marks of its test functions"""
    import test_gpu_draw_edges as G

    def names(fn):
        return [list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "name"][0]
    assert G.CASE_LISTS == D.ENTRY_LISTS
    assert G.FORMS == ("draw only", "mix then draw", "mix only, then draw only")
    collected = {"channel draw": names(G.test_channel_draw_only), "channel mix+draw": names(G.test_channel_mix_then_draw),
                 "fri commit": names(G.test_fri_commit_layers), "gkr round_finish": names(G.test_gkr_round_finish),
                 "gkr layer_begin": names(G.test_gkr_layer_begin), "gkr layer_end": names(G.test_gkr_layer_end),
                 "gkr prove_batch": names(G.test_gkr_prove_batch)}
    assert collected == D.ENTRY_LISTS
    through_the_prover = names(G.test_fri_prover_and_verifier_across_a_draw)
    assert through_the_prover == [c.name for c in D.CASES if c.entry == "fri" and c.target < 2]


# ---------------------------------------------------------------- the search tool, as a program of its own under sanitizers
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("draw_edge_search") / "draw_edge_search")
    subprocess.check_call(["cc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I",
                           os.path.join(ROOT, "oracle"), "-o", out, os.path.join(ROOT, "tools", "draw_edge_search.c"),
                           os.path.join(ROOT, "oracle", "tstwo_oracle.c")])
    return out


def run_tool(tool, args):
    r = subprocess.run([tool] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return json.loads(r.stdout)


def test_search_tool_short_run_is_clean_and_deterministic(tool, tmp_path):
    case = D.BY_NAME["mix/rej_hi_2P"]
    args = D.search_arguments(case, str(tmp_path)) + ["--salt", str(D.salt(case)), "--bound", str(1 << 20)]
    first, again = run_tool(tool, args), run_tool(tool, args)
    assert first == again and first["trials"] <= 1 << 20
    assert not first["found"] and first["trials"] == 1 << 20 and first["checksum"] > 0       # 2^20 trials at 2^-30: recorded, not luck
    # fewer lanes walk other digests: the report says so through its checksum
    assert run_tool(tool, args + ["--lanes", "3"])["checksum"] != first["checksum"]


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_search_tool_reports_the_fixture_at_its_counter(tool, tmp_path, name):
    case, fx = D.BY_NAME[name], FIX[name]
    s = fx["search"]
    rep = run_tool(tool, D.search_arguments(case, str(tmp_path)) + ["--salt", str(s["salt"]), "--lane", str(s["lane"]), "--start",
                                                                     str(s["counter"]), "--bound", "1"])
    assert rep["found"] and rep["digest"] == fx["state"][:8] and rep["trials"] == 1
    assert (rep["word"], rep["value"]) == (fx["cond"]["word"], fx["cond"]["value"])
    before = run_tool(tool, D.search_arguments(case, str(tmp_path)) + ["--salt", str(s["salt"]), "--lane", str(s["lane"]), "--start",
                                                                        str(max(s["counter"] - 1, 0)), "--bound", "1"])
    assert s["counter"] == 0 or not before["found"]
