"""The proof-of-work searches without a GPU: csrc/grind_plan.h, compiled on its own with the address and undefined behaviour
sanitizers, against the tests' own statement (tests/grind_plan.py); the oracle's sequential scan against hashlib and the host
channel; every Blake2s constant of tests/grind_cases.py re-derived by that scan; and the conditions that keep the cases from being
vacuous: a hit on both sides of every batch edge, high-word answers that a search mixing the wrong words cannot give."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

import grind_cases as GC
import grind_plan as GP
import poseidon_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "tstwo_amd", "csrc")
NONE = GP.NONE


# ---------------------------------------------------------------- the header against its restatement
def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/grind_plan_main.cpp — csrc/grind_plan.h and nothing else of the library — under the address and undefined behaviour
    sanitizers."""
    out = str(tmp_path_factory.mktemp("grind_plan") / "grind_plan_main")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "grind_plan_main.cpp"), "-o", out])
    return out


def _library_lines(exe, lines):
    p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.splitlines()
    assert len(got) == len(lines)
    return got


def _own(kind, start, n_max):
    b = GP.batches(kind, start, n_max)
    words = [f"{base}:{count}" for base, count in b]
    if len(b) < n_max or b[-1][0] + b[-1][1] == NONE:          # the call after the last batch returns 0
        words.append("exhausted")
    return " ".join(words)


PLAN_STARTS = [0, 1, 12345, 2**32 - 3, 2**40 + 7, 2**63,
               NONE - 2**20 - 1, NONE - 2**20, NONE - 2**20 + 1, NONE - 5 * 2**20 - 3, NONE - 2**26, NONE - 2**26 - 2**22 - 1, NONE - 2**26 - 2**22 + 1,
               NONE - 2**16, NONE - 2**16 - 2**18 - 77, NONE - 2**23,
               NONE - 300, NONE - 258, NONE - 257, NONE - 256, NONE - 101, NONE - 2, NONE - 1, NONE]


def test_header_equals_the_restated_schedule(exe):
    cases = [(kind, start, n_max) for kind in GP.KINDS for start in PLAN_STARTS for n_max in (1, 5, 9)]
    got = _library_lines(exe, [f"B {GP.KINDS[kind]} {start} {n_max}" for kind, start, n_max in cases])
    for case, line in zip(cases, got):
        assert line == _own(*case), case


def test_header_constants(exe):
    got = [int(w) for w in _library_lines(exe, ["C"])[0].split()]
    assert got == [NONE, GP.LANES, 1 << 20, 1 << 22, 1 << 26, 1 << 16, 2, 1 << 22]


def test_schedule_written_out():
    """The two schedules by hand, and the properties the kernels rely on: batches tile the range without gap or overlap, none holds
    2^64 - 1, each fits a 32-bit grid, and only a batch that ends at 2^64 - 2 is not a multiple of the workgroup."""
    M = 1 << 20
    assert GP.batches(GP.BLAKE2S, 5, 6) == [(5, M), (5 + M, M), (5 + 2 * M, M), (5 + 3 * M, M), (5 + 4 * M, 64 * M), (5 + 68 * M, 64 * M)]
    assert GP.batches(GP.P252, 5, 6) == [(5, 1 << 16), (5 + (1 << 16), 1 << 18), (5 + 5 * (1 << 16), M), (5 + 21 * (1 << 16), 4 * M),
                                         (5 + 85 * (1 << 16), 4 * M), (5 + 149 * (1 << 16), 4 * M)]
    assert GP.batches(GP.BLAKE2S, NONE - 2, 9) == [(NONE - 2, 2)] and GP.batches(GP.P252, NONE - 258, 9) == [(NONE - 258, 258)]
    assert GP.batches(GP.BLAKE2S, NONE, 9) == [] and GP.batches(GP.P252, NONE, 9) == []
    assert GP.edges(GP.BLAKE2S, 4 * M) == [M, 2 * M, 3 * M, 4 * M] and GP.first_grown_edge(GP.BLAKE2S) == 4 * M
    assert GP.edges(GP.P252, 5 * (1 << 16)) == [1 << 16, 5 * (1 << 16)] and GP.first_grown_edge(GP.P252) == 1 << 16
    for kind in GP.KINDS:
        for start in PLAN_STARTS:
            at = start
            for base, count in GP.batches(kind, start, 12):
                assert base == at and 0 < count and base + count <= NONE
                assert -(-count // GP.LANES) < 2**32
                assert count % GP.LANES == 0 or base + count == NONE
                at = base + count
    assert GP.idle_lane_nonces(NONE - 2, 2) == [NONE] + list(range(253)) and GP.idle_lane_nonces(7, 512) == []


# ---------------------------------------------------------------- the oracle's scan
def test_oracle_scan_equals_hashlib_and_the_host_channel():
    """orc_grind_blake2s nonce by nonce (limit 1: does this nonce qualify?) against hashlib and against Blake2sChannel.mix_u64 /
    trailing_zeros, a few hundred nonces, a third of them with a non-zero high word."""
    ch = GC.blake2s_channel(7)
    d = GC.digest(7)
    nonces = list(range(150)) + [2**32 - 2 + i for i in range(50)] + [(0x9E3779B97F4A7C15 * (i + 1)) % 2**64 for i in range(100)] + [NONE - 1, NONE]
    assert sum(n >> 32 != 0 for n in nonces) >= 100
    seen = set()
    for n in nonces:
        h = hashlib.blake2s(d + n.to_bytes(8, "little")).digest()
        v = int.from_bytes(h[:16], "little")
        tz = 128 if v == 0 else (v & -v).bit_length() - 1
        c = ch.clone()
        c.mix_u64(n)
        assert c.digest() == h and c.trailing_zeros() == tz
        seen.add(min(tz, 4))
        assert orc.grind_blake2s(d, tz, n, 1) == n and orc.grind_blake2s(d, tz + 1, n, 1) is None, n
    assert seen == {0, 1, 2, 3, 4}


def test_oracle_scan_is_the_sequential_loop():
    d, ch = GC.digest(8), GC.blake2s_channel(8)
    for pow_bits, start in [(0, 17), (3, 0), (6, 1000), (9, 2**32 - 100), (10, 2**40 + 2**32 - 2), (3, NONE - 40)]:
        want = GC.host_grind(ch, pow_bits, start, min(start + 8192, 2**64))
        assert want is not None and orc.grind_blake2s(d, pow_bits, start, 8192) == want
        assert orc.grind_blake2s(d, pow_bits, start, want - start) is None          # the limit counts nonces
    assert orc.grind_blake2s(d, 129, NONE - 10, 1000) is None                       # stops at 2^64 - 1, no wrap


# ---------------------------------------------------------------- the constants, re-derived
@pytest.fixture(scope="module")
def anchor_scans():
    """(first hit from 0, first hit from behind it) of each Blake2s anchor, by the oracle's loop within CAP nonces each."""
    out = []
    for a in GC.B2_ANCHORS:
        d = GC.digest(a["seed"])
        first = orc.grind_blake2s(d, a["pow_bits"], 0, GC.CAP)
        out.append((first, None if first is None else orc.grind_blake2s(d, a["pow_bits"], first + 1, GC.CAP)))
    return out


def test_blake2s_anchors_are_first_hits(anchor_scans):
    assert len(GC.B2_ANCHORS) == 2
    for a, (first, nxt) in zip(GC.B2_ANCHORS, anchor_scans):
        assert (first, nxt) == (a["first"], a["next"])
        assert GC.B2_ANCHOR_MIN < first <= GC.CAP and nxt is not None
        for n in (first, nxt):                                           # and by hashlib
            assert GC.qualifies(GC.blake2s_channel(a["seed"]), a["pow_bits"], n)
        assert all(first - k >= 0 for k in GC.B2_ANCHOR_K)


def test_every_batch_edge_has_a_hit_on_either_side():
    """For each schedule, every batch edge e up to the beginning of the first grown batch (and, as far as the anchor reaches, behind
    it) has a start that puts the hit at offset e - 1, the last lane of a batch, and one that puts it at e, lane 0 of the next.  If
    the batch sizes change, this fails until the cases move."""
    for kind, ks, reach in ((GP.BLAKE2S, GC.B2_ANCHOR_K, GC.B2_ANCHOR_MIN), (GP.P252, GC.P252_ANCHOR_K, GC.P252_ANCHOR_MIN)):
        edges = GP.edges(kind, reach)
        assert GP.first_grown_edge(kind) in edges and len(edges) >= 2
        for e in edges:
            assert e - 1 in ks and e in ks, (kind, e)
        assert GP.first_grown_edge(kind) + 1 in ks
    assert GC.P252_ANCHOR_MIN < GC.P252_ANCHOR["first"] <= GC.P252_ANCHOR_MAX
    assert GC.P252_ANCHOR["first"] < GC.P252_ANCHOR["next"] <= GC.P252_ANCHOR["first"] + (1 << 20)


HIGH = [("blake2s", GC.blake2s_channel, s, p) for s, p in GC.B2_HIGH] + [("p252", GC.p252_channel, s, p) for s, p in GC.P252_HIGH]


def test_high_word_cases_are_listed():
    assert {p for _, p in GC.B2_HIGH} <= {4, 8, 12} and len(GC.B2_HIGH) >= 2
    assert {p for _, p in GC.P252_HIGH} <= {2, 4} and len(GC.P252_HIGH) >= 1
    assert GC.HIGH_STARTS == [2**32 - 3, 2**32 - 1, 2**32, 2**33 + 5, 2**40 + 2**32 - 2, 2**63, 2**64 - 2**21]


@pytest.mark.parametrize("hash_name,channel_of,seed,pow_bits", HIGH)
def test_high_word_cases_are_not_vacuous(hash_name, channel_of, seed, pow_bits):
    """Every answer differs from the one to start & 0xFFFFFFFF and, which is what counts, from what a search returns that mixes
    only the low word, or the two words swapped; the answers from below 2^32 lie at or above it."""
    ch = channel_of(seed)
    for start in GC.HIGH_STARTS:
        answer = GC.host_grind(ch, pow_bits, start, start + 4096)
        assert answer is not None and answer >= 2**32
        low = start & 0xFFFFFFFF
        if low != start:                             # (from below 2^32 the two searches are one: there the crossing is what counts)
            assert answer != GC.host_grind(ch, pow_bits, low, low + 4096)
        for what, mixed in GC.MIX_FAULTS.items():
            assert GC.host_grind(ch, pow_bits, start, answer + 1, mixed) != answer, (start, what)


END = [("blake2s", GC.blake2s_channel, GC.B2_END_HIT, GC.B2_END_EXHAUSTED), ("p252", GC.p252_channel, GC.P252_END_HIT, GC.P252_END_EXHAUSTED)]


@pytest.mark.parametrize("hash_name,channel_of,hit,exhausted", END)
def test_end_of_space_cases(hash_name, channel_of, hit, exhausted):
    """start = 2^64 - 1 - m: the one batch is [start, 2^64 - 2].  The hit cases have a nonce in it that qualifies, not the first one
    where there is room; the exhausted cases have none, but one among the nonces the idle lanes would compute."""
    assert sorted(hit) == sorted(exhausted) == GC.END_M == [1, 100, 257]
    for m in GC.END_M:
        start = NONE - 1 - m
        assert GP.batches(GP.BLAKE2S, start, 9) == GP.batches(GP.P252, start, 9) == [(start, m + 1)]
        seed, pow_bits = hit[m]
        answer = GC.host_grind(channel_of(seed), pow_bits, start)
        assert answer is not None and (answer > start or m == 1)
        seed, pow_bits = exhausted[m]
        ch = channel_of(seed)
        assert GC.host_grind(ch, pow_bits, start) is None
        idle = GP.idle_lane_nonces(start, m + 1)
        assert idle[0] == NONE and idle[1] == 0 and len(idle) == -(m + 1) % GP.LANES
        assert any(GC.qualifies(ch, pow_bits, n) for n in idle[1:])       # a wrapped one: an atomicMin would prefer it
        if hash_name == "blake2s":
            assert orc.grind_blake2s(GC.digest(seed), pow_bits, start, m + 1) is None
            assert orc.grind_blake2s(GC.digest(hit[m][0]), hit[m][1], start, m + 1) == answer


def test_pow32_case_by_hashlib():
    """One hash: the recorded answer qualifies; the 2^20 nonces below it do not (the oracle's loop).  That no nonce between the
    start and the answer qualifies is not claimed: 2^32 hashes are out of a CPU loop's reach."""
    c = GC.B2_POW32
    d = GC.digest(c["seed"])
    h = hashlib.blake2s(d + c["answer"].to_bytes(8, "little")).digest()
    assert h[:4] == bytes(4)
    assert c["start"] + (1 << 22) + 24 * (1 << 26) <= c["answer"] < 2**33              # dozens of 2^26 batches
    assert orc.grind_blake2s(d, 32, c["answer"] - (1 << 20), 1 << 20) is None


def test_channel_tz_equals_the_model():
    vals = [0, 1, 1 << 248, 1 << 249, 3 << 254, 1 << 240, 1 << 224, 1 << 216, 1 << 192, 1 << 128, 1 << 127, (1 << 256) - 1, PM.P - 1]
    words = np.array([PM.to_words(v) for v in vals], dtype=np.uint32)
    assert GC.channel_tz(words).tolist() == [PM.trailing_zeros(v) for v in vals]
