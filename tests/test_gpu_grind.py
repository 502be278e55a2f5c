"""tstwo_grind_blake2s and tstwo_grind_poseidon252 called by name on the MI355X with the raw arguments, at the cases of
tests/grind_cases.py: start nonces that put the hit on either side of every batch edge of the host schedule, nonces with a high
word, the last nonces below 2^64 - 1, the refusals, pow_bits = 32.  tests/test_cpu_grind.py shows that the cases test what they are
meant to; the references here are its constants, the host's sequential loop, and for the Poseidon anchor tstwo_poseidon252_hash_many
over the whole range, sampled against tests/poseidon_model.py."""
import ctypes as C
import hashlib
import time

import numpy as np
import pytest

import grind_cases as GC
import poseidon_model as M
import tstwo_amd as T
from gpu_util import dev
from oracle import oracle as orc
from tstwo_amd import _lib as L
from tstwo_amd.poseidon import grind_poseidon252

pytestmark = pytest.mark.gpu

NONE = GC.NONE
BAD_ARG = 7          # TSTWO_ERR_BAD_ARG


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def b2_raw(digest, pow_bits, start):
    d = np.frombuffer(digest, dtype=np.uint8).copy()
    out = C.c_uint64(0xDEAD)
    L.call("tstwo_grind_blake2s", d.ctypes.data_as(L.u8p), pow_bits, start, C.byref(out))
    return out.value


def p252_raw(digest, pow_bits, start):
    d = np.array(M.to_words(digest), dtype=np.uint32)
    out = C.c_uint64(0xDEAD)
    L.call("tstwo_grind_poseidon252", d.ctypes.data_as(L.u32p), pow_bits, start, C.byref(out))
    return out.value


def b2(seed, pow_bits, start):
    return b2_raw(GC.digest(seed), pow_bits, start)


def p252(seed, pow_bits, start):
    return p252_raw(GC.p252_digest(seed), pow_bits, start)


def refused(fn, *args, match):
    with pytest.raises(L.TstwoError, match=match) as e:
        fn(*args)
    assert e.value.code == BAD_ARG


# ---------------------------------------------------------------- Blake2s: start nonces and batch edges
@pytest.mark.parametrize("anchor", GC.B2_ANCHORS, ids=lambda a: f"seed{a['seed']}")
def test_blake2s_first_hit_from_every_start(anchor):
    """No nonce below `first` qualifies (a full CPU scan, tests/test_cpu_grind.py), so every start in (first - k) returns first: the
    hit on lane 0, on the last lane of a batch, on lane 0 of the next, in the first 2^26 batch."""
    seed, pow_bits, first = anchor["seed"], anchor["pow_bits"], anchor["first"]
    assert b2(seed, pow_bits, 0) == first
    for k in GC.B2_ANCHOR_K:
        assert b2(seed, pow_bits, first - k) == first, k
    assert b2(seed, pow_bits, first + 1) == anchor["next"]


# ---------------------------------------------------------------- the high word
@pytest.mark.parametrize("seed,pow_bits", GC.B2_HIGH)
def test_blake2s_high_word(seed, pow_bits):
    ch = GC.blake2s_channel(seed)
    for start in GC.HIGH_STARTS:
        assert b2(seed, pow_bits, start) == GC.host_grind(ch, pow_bits, start), start


@pytest.mark.parametrize("seed,pow_bits", GC.P252_HIGH)
def test_poseidon252_high_word(seed, pow_bits):
    ch = GC.p252_channel(seed)
    for start in GC.HIGH_STARTS:
        assert p252(seed, pow_bits, start) == GC.host_grind(ch, pow_bits, start), start


# ---------------------------------------------------------------- the end of the nonce space
END = [(b2, GC.blake2s_channel, GC.B2_END_HIT, GC.B2_END_EXHAUSTED), (p252, GC.p252_channel, GC.P252_END_HIT, GC.P252_END_EXHAUSTED)]


@pytest.mark.parametrize("grind,channel_of,hit,exhausted", END, ids=["blake2s", "poseidon252"])
def test_last_batch_below_two_to_the_64(grind, channel_of, hit, exhausted):
    """start = 2^64 - 1 - m: one batch of m + 1 nonces, the only kind that does not fill its last workgroup.  Its idle lanes would
    compute 2^64 - 1, 0, 1, ...; in the exhausted cases one of those qualifies and none of [start, 2^64 - 2] does."""
    for m in GC.END_M:
        start = NONE - 1 - m
        assert grind(7, 0, start) == start
        seed, pow_bits = hit[m]
        assert grind(seed, pow_bits, start) == GC.host_grind(channel_of(seed), pow_bits, start), m
        seed, pow_bits = exhausted[m]
        refused(grind, seed, pow_bits, start, match="nonce space exhausted")
        assert grind(seed, pow_bits, start - 4096) == GC.host_grind(channel_of(seed), pow_bits, start - 4096)      # and answers again
    for pow_bits in (0, 1):
        refused(grind, 7, pow_bits, NONE, match="nonce space exhausted")              # 2^64 - 1 itself is never tried


# ---------------------------------------------------------------- refusals
def test_blake2s_refusals_leave_the_next_call_right():
    a = GC.B2_ANCHORS[0]
    d = np.frombuffer(GC.digest(a["seed"]), dtype=np.uint8).copy()
    out = C.c_uint64(0xDEAD)
    for bad in (lambda: b2(a["seed"], 129, 0),
                lambda: L.call("tstwo_grind_blake2s", None, 1, 0, C.byref(out)),
                lambda: L.call("tstwo_grind_blake2s", d.ctypes.data_as(L.u8p), 1, 0, None)):
        refused(bad, match="grind: ")
        assert out.value == 0xDEAD
        assert b2(a["seed"], a["pow_bits"], a["first"] - 300) == a["first"]


def test_pow_bits_128_is_accepted_and_exhausts():
    refused(b2, 7, 128, NONE - 600, match="nonce space exhausted")
    refused(p252, 7, 128, NONE - 600, match="nonce space exhausted")


def test_poseidon252_refusals_leave_the_next_call_right():
    seed, pow_bits = GC.P252_HIGH[0]
    want = GC.host_grind(GC.p252_channel(seed), pow_bits, 2**33 + 5)
    dw = np.array(M.to_words(GC.p252_digest(seed)), dtype=np.uint32)
    out = C.c_uint64(0xDEAD)
    top_limb_only = (M.to_words(M.P)[7] + 1) << 224                                # limbs 0..6 zero, limb 7 above p's
    for bad in (lambda: p252(seed, 129, 0),
                lambda: L.call("tstwo_grind_poseidon252", None, 1, 0, C.byref(out)),
                lambda: L.call("tstwo_grind_poseidon252", dw.ctypes.data_as(L.u32p), 1, 0, None),
                lambda: p252_raw(M.P, 1, 0), lambda: p252_raw(M.P + 1, 1, 0), lambda: p252_raw(top_limb_only, 1, 0)):
        refused(bad, match="grind: ")
        assert out.value == 0xDEAD
        assert p252(seed, pow_bits, 2**33 + 5) == want
    assert p252_raw(M.P - 1, 0, 5) == 5                                             # the largest canonical digest passes


# ---------------------------------------------------------------- Blake2s, pow_bits = 32
def test_blake2s_pow_bits_32():
    """The first digest word is zero and the second decides: `else if (h[1])` of the kernel, dozens of 2^26 batches.  Checked: the
    answer qualifies (one hashlib hash), is the recorded one, is not below the start, is returned again from start = answer, and
    none of the 2^20 nonces below it qualifies (the oracle's loop).  NOT checked: that no nonce between the start and the answer
    qualifies — a CPU loop over 2^32 hashes is out of reach, so this case does not claim full minimality."""
    c = GC.B2_POW32
    d = GC.digest(c["seed"])
    t = time.perf_counter()
    answer = b2_raw(d, 32, c["start"])
    print(f"pow_bits 32 from {c['start']}: nonce {answer} in {(time.perf_counter() - t) * 1e3:.1f} ms")
    h = hashlib.blake2s(d + answer.to_bytes(8, "little")).digest()
    v = int.from_bytes(h[:16], "little")
    assert v != 0 and (v & -v).bit_length() - 1 >= 32
    assert answer >= c["start"] and answer == c["answer"]
    assert b2_raw(d, 32, answer) == answer
    assert orc.grind_blake2s(d, 32, answer - (1 << 20), 1 << 20) is None


# ---------------------------------------------------------------- Poseidon252: the anchor
@pytest.fixture(scope="module")
def anchor_hashes():
    """hash_many([digest, nonce]) for every nonce in [0, next hit] in one call: rows of 8 limbs."""
    a = GC.P252_ANCHOR
    n = a["next"] + 1
    assert n <= (1 << 21)
    msgs = np.zeros((n, 16), dtype=np.uint32)
    msgs[:, :8] = M.to_words(GC.p252_digest(a["seed"]))
    msgs[:, 8] = np.arange(n, dtype=np.uint64) & 0xFFFFFFFF
    src, dst = dev(msgs.reshape(-1)), L.DeviceBuffer(32 * n)
    L.call("tstwo_poseidon252_hash_many", C.c_void_p(src.ptr), n, 2, C.c_void_p(dst.ptr))
    out = dst.download(np.uint32).reshape(-1, 8)
    out.setflags(write=False)
    return out


def test_poseidon252_anchor_is_the_first_hit(anchor_hashes):
    a = GC.P252_ANCHOR
    first, nxt, pow_bits = a["first"], a["next"], a["pow_bits"]
    assert GC.P252_ANCHOR_MIN < first <= GC.P252_ANCHOR_MAX and first < nxt <= first + (1 << 20)
    assert p252(a["seed"], pow_bits, 0) == first
    hits = np.nonzero(GC.channel_tz(anchor_hashes) >= pow_bits)[0].tolist()
    assert hits == [first, nxt]
    # the reference kernel against the model: the hits, both sides of the batch edges, a spread
    d = GC.p252_digest(a["seed"])
    sample = {first, nxt, 0, 1, first - 1, first + 1} | {e + s for e in (1 << 16, (1 << 16) + (1 << 18)) for s in (-1, 0)}
    rng = np.random.default_rng(19)
    sample |= set(rng.integers(0, nxt, size=64 - len(sample)).tolist())
    for n in sorted(sample):
        assert M.from_words(anchor_hashes[n]) == M.hash_many([d, n]), n
    assert M.trailing_zeros(M.hash_many([d, first])) >= pow_bits


def test_poseidon252_first_hit_from_every_start():
    a = GC.P252_ANCHOR
    for k in GC.P252_ANCHOR_K:
        assert p252(a["seed"], a["pow_bits"], a["first"] - k) == a["first"], k
    assert p252(a["seed"], a["pow_bits"], a["first"] + 1) == a["next"]


# ---------------------------------------------------------------- the wrappers at a non-zero start
def test_wrappers_pass_the_start_nonce():
    a = GC.B2_ANCHORS[0]
    ch = GC.blake2s_channel(a["seed"])
    assert T.grind(ch, a["pow_bits"], start_nonce=a["first"] - 256) == a["first"]
    assert T.HipGrindOps.grind(ch, a["pow_bits"], a["first"] + 1) == a["next"]
    seed, pow_bits = GC.P252_HIGH[0]
    pc = GC.p252_channel(seed)
    want = GC.host_grind(pc, pow_bits, 2**32 - 3)
    assert T.grind(pc, pow_bits, start_nonce=2**32 - 3) == want == grind_poseidon252(pc, pow_bits, 2**32 - 3)
    assert T.grind(pc, pow_bits) == GC.host_grind(pc, pow_bits, 0)
