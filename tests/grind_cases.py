"""The named cases of the proof-of-work tests, shared by tests/test_cpu_grind.py (which re-derives every constant below that a CPU
loop can reach) and tests/test_gpu_grind.py (which sends each case through the C entries).

A case's channel digest is blake2s(b"grind-case-<seed>"): as it stands for Blake2s, as the little-endian integer mod p (8 limbs) for
Poseidon252.  References are sequential loops: the oracle's orc_grind_blake2s for full scans, and `host_grind` below — the
reference's loop (backend/cpu/grind.ts:31-42: mix_u64 on a clone, then trailing_zeros) over the host channel classes — for the rest.
Trailing zeros past the first 32-bit word of a Poseidon digest (pow_bits > 32) cannot be reached by a search and are left out."""
import hashlib

import numpy as np

from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.poseidon import STARKNET_PRIME, FieldElement252, Poseidon252Channel

import grind_plan as GP

NONE = GP.NONE
CAP = 1 << 24                 # the most nonces one CPU scan of a Blake2s case walks


def digest(seed):
    return hashlib.blake2s(b"grind-case-%d" % seed).digest()


def p252_digest(seed):
    return int.from_bytes(digest(seed), "little") % STARKNET_PRIME


def blake2s_channel(seed):
    ch = Blake2sChannel(ts_compat=False)
    ch._digest = digest(seed)
    return ch


def p252_channel(seed):
    return Poseidon252Channel(FieldElement252(p252_digest(seed)))


def qualifies(channel, pow_bits, nonce):
    c = channel.clone()
    c.mix_u64(nonce)
    return c.trailing_zeros() >= pow_bits


def host_grind(channel, pow_bits, start, stop=NONE, mixed=lambda n: n):
    """The first nonce in [start, stop) that qualifies, or None.  `mixed`: what a faulty search would mix in place of the nonce."""
    for n in range(start, stop):
        if qualifies(channel, pow_bits, mixed(n)):
            return n
    return None


def channel_tz(words):
    """Trailing zeros as channel/poseidon.ts:209-229 counts them, of elements given as rows of 8 little-endian limbs: the first 16
    bytes of the big-endian encoding — limbs 7, 6, 5, 4, each byte-swapped — as a little-endian u128."""
    tz = np.full(len(words), 128, dtype=np.int64)
    for j, limb in reversed(list(enumerate((7, 6, 5, 4)))):
        w = words[:, limb].astype(np.uint32).byteswap().astype(np.int64)
        low = w & -w
        tz = np.where(w != 0, 32 * j + np.round(np.log2(np.maximum(low, 1))).astype(np.int64), tz)
    return tz


# What a search returns that mixes a wrong word pair for nonce n: the high word dropped, the two words swapped.
MIX_FAULTS = {"high word dropped": lambda n: n & 0xFFFFFFFF, "words swapped": lambda n: (n >> 32) | ((n & 0xFFFFFFFF) << 32)}

# ---------------------------------------------------------------- anchors: first hits from 0, proven minimal by a full scan
# Blake2s: 2^22 + 2^20 < first <= 2^24, so that first - k >= 0 for every k below and a CPU scan of [0, first] stays within CAP.
# next: the first hit from first + 1 (within CAP nonces).
B2_ANCHORS = [
    {"seed": 0, "pow_bits": 23, "first": 6544835, "next": 9652611},
    {"seed": 3, "pow_bits": 22, "first": 6860325, "next": 8555242},
]
_M = 1 << 20
# start = first - k must return first: the hit sits k lanes behind the start.  k = e - 1 / e for a batch edge e (grind_plan.edges)
# puts it on the last lane of a batch / on lane 0 of the next; 4 * 2^20 is lane 0 of the first 2^26 batch.
B2_ANCHOR_K = [0, 1, 255, 256, _M - 1, _M, _M + 1, 2 * _M - 1, 2 * _M, 3 * _M - 1, 3 * _M, 4 * _M - 1, 4 * _M, 4 * _M + 1]
B2_ANCHOR_MIN = 4 * _M + _M                 # first must exceed this: 2^22 + 2^20

# Poseidon252: 2^16 + 2^18 < first <= 2^20.  The channel counts from bit 248 of an element below 2^252, so the first byte it reads
# is 0 in one digest of eight and 8 of the bits come at the price of 3: pow_bits 23 is as hard as 18 bits.  The full-range reference
# is tstwo_poseidon252_hash_many over [0, next], itself tied to tests/poseidon_model.py; first and next were found on the MI355X and
# are asserted, not assumed, by the GPU test.
P252_ANCHOR = {"seed": 202, "pow_bits": 23, "first": 457247, "next": 618787}
_A, _B = 1 << 16, (1 << 16) + (1 << 18)
P252_ANCHOR_K = [0, 1, _A - 1, _A, _A + 1, _B - 1, _B, _B + 1]
P252_ANCHOR_MIN, P252_ANCHOR_MAX = _B, 1 << 20

# ---------------------------------------------------------------- the high word of the nonce
HIGH_STARTS = [2**32 - 3, 2**32 - 1, 2**32, 2**33 + 5, 2**40 + 2**32 - 2, 2**63, 2**64 - 2**21]
# (seed, pow_bits): every start above goes with each.  Seeds were chosen so that the answers from 2^32 - 3 and 2^32 - 1 lie at or
# above 2^32, and so that no answer is what a search with one of MIX_FAULTS returns (tests/test_cpu_grind.py asserts both).
B2_HIGH = [(11, 4), (12, 8), (15, 12)]
P252_HIGH = [(31, 2), (37, 4)]

# ---------------------------------------------------------------- the end of the nonce space: start = 2^64 - 1 - m
END_M = [1, 100, 257]
# m -> (seed, pow_bits) with a qualifying nonce in [start, 2^64 - 2]
B2_END_HIT = {1: (50, 1), 100: (52, 5), 257: (56, 5)}
P252_END_HIT = {1: (70, 1), 100: (72, 5), 257: (77, 5)}
# m -> (seed, pow_bits) with none in [start, 2^64 - 2], but with one among the small nonces that the idle lanes of the last
# workgroup would reach past 2^64 - 1 if they ran (grind_plan.idle_lane_nonces): the search must fail with "nonce space exhausted".
# One nonce in 128 qualifies: 7 bits for Blake2s, 12 for Poseidon252 (see P252_ANCHOR on its first 8 bits).
B2_END_EXHAUSTED = {1: (51, 7), 100: (55, 7), 257: (57, 7)}
P252_END_EXHAUSTED = {1: (71, 12), 100: (76, 12), 257: (78, 12)}

# ---------------------------------------------------------------- Blake2s at pow_bits = 32: the second digest word decides
# answer: found on the MI355X (profiles/grind_cases.txt); below 2^33, dozens of 2^26 batches behind the start.
B2_POW32 = {"seed": 106, "pow_bits": 32, "start": 12345, "answer": 5259451497}
