"""The Poseidon252 Merkle channel (vcs/poseidon252_merkle.ts, channel/poseidon.ts, backend/cpu/poseidon252.ts): the channel a proof
uses when it is to be verified on Starknet.

Trees and the proof-of-work grind run on the GPU (csrc/poseidon.hip); the channel and the verifier's hashNode need a handful of
hashes and stay on the host, in Python integers — except inside a FRI commit, whose transcript can run on the device
(DevicePoseidon252Channel, csrc/poseidon_coop.hip).  Poseidon here is Starknet's: Hades over F_p, p = 2^251 + 17 2^192 + 1, width 3,
8 full and 83 partial rounds, S-box x^3; poseidonHashMany / poseidonHash as @scure/starknet computes them for the reference.

A FieldElement252 crosses the C ABI and lives in device memory as 8 little-endian u32 limbs (32 bytes): a Poseidon tree has the
layout of a Blake2s tree, so the decommitment entries of the library serve both.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

from . import _lib as L
from .backend import _vp
from .fields import M31, P as M31_P
from .vcs import DeviceHashLayer, MerkleProver, _LazyList

STARKNET_PRIME = 2**251 + 17 * 2**192 + 1
BYTES_PER_FELT252 = 31
FELTS_PER_HASH = 8
ELEMENTS_IN_BLOCK = 8
SECURE_EXTENSION_DEGREE = 4
_MAX_U32 = 0xFFFFFFFF


class FieldElement252:
    """channel/poseidon.ts:28-111: an element of the Starknet field, immutable."""
    __slots__ = ("_v",)

    def __init__(self, value: int):
        if not 0 <= value < STARKNET_PRIME:
            raise TypeError(f"Value must be in range [0, {STARKNET_PRIME})")
        self._v = value

    @staticmethod
    def zero() -> "FieldElement252":
        return FieldElement252(0)

    @staticmethod
    def from_(value: int) -> "FieldElement252":
        return FieldElement252(int(value) % STARKNET_PRIME)

    @staticmethod
    def fromHexBe(h: str):
        try:
            return FieldElement252(int(h if h.startswith("0x") else "0x" + h, 16) % STARKNET_PRIME)
        except ValueError:
            return None

    @staticmethod
    def from_words(words) -> "FieldElement252":
        """8 little-endian u32 limbs (the device / C-ABI representation)."""
        return FieldElement252(sum(int(w) << (32 * k) for k, w in enumerate(words)))

    @staticmethod
    def from_le_bytes(b: bytes) -> "FieldElement252":
        return FieldElement252(int.from_bytes(bytes(b), "little"))

    def add(self, o): return FieldElement252((self._v + o._v) % STARKNET_PRIME)
    def sub(self, o): return FieldElement252((self._v - o._v) % STARKNET_PRIME)
    def mul(self, o): return FieldElement252((self._v * o._v) % STARKNET_PRIME)

    def floorDiv(self, o) -> "FieldElement252":
        if o._v == 0:
            raise ValueError("Division by zero")
        return FieldElement252(self._v // o._v)

    def toBigInt(self) -> int: return self._v
    def toBytesBe(self) -> bytes: return self._v.to_bytes(32, "big")
    asBytes = toBytesBe
    def to_le_bytes(self) -> bytes: return self._v.to_bytes(32, "little")
    def to_words(self) -> list: return [(self._v >> (32 * k)) & _MAX_U32 for k in range(8)]
    def tryIntoU32(self): return self._v if self._v <= _MAX_U32 else None
    def tryIntoU8(self): return self._v if self._v <= 0xFF else None
    def equals(self, o) -> bool: return isinstance(o, FieldElement252) and o._v == self._v
    def __eq__(self, o): return self.equals(o)
    def __hash__(self): return hash(self._v)
    def __int__(self): return self._v
    def __repr__(self): return f"FieldElement252({hex(self._v)})"


setattr(FieldElement252, "from", FieldElement252.from_)        # the reference's name (a keyword in Python)


# ---- Starknet Poseidon on the host (the device twin is csrc/felt252.cuh + poseidon.hip)
def _round_constants() -> tuple:
    """Public definition: ARK[i][j] = sha256("Hades" + str(3 i + j)) as a big-endian integer, mod p."""
    return tuple(tuple(int.from_bytes(hashlib.sha256(b"Hades%d" % (3 * i + j)).digest(), "big") % STARKNET_PRIME for j in range(3))
                 for i in range(91))


_ARK = _round_constants()
_FULL = frozenset(range(4)) | frozenset(range(87, 91))


def hades_permutation(s0: int, s1: int, s2: int) -> tuple:
    p = STARKNET_PRIME
    for r, (c0, c1, c2) in enumerate(_ARK):
        s0, s1, s2 = s0 + c0, s1 + c1, (s2 + c2) % p
        if r in _FULL:
            s0, s1 = s0 % p, s1 % p
            s0, s1 = s0 * s0 % p * s0 % p, s1 * s1 % p * s1 % p
        s2 = s2 * s2 % p * s2 % p
        t = s0 + s1 + s2
        s0, s1, s2 = (t + 2 * s0) % p, (t - 2 * s1) % p, (t - 3 * s2) % p
    return s0, s1, s2


def poseidon_hash_many(values) -> int:
    """poseidonHashMany: append 1, then 0 to an even length; absorb pairs into s0, s1 and permute; the hash is s0."""
    v = [int(x) for x in values] + [1]
    if len(v) & 1:
        v.append(0)
    s0 = s1 = s2 = 0
    for i in range(0, len(v), 2):
        s0, s1, s2 = hades_permutation((s0 + v[i]) % STARKNET_PRIME, (s1 + v[i + 1]) % STARKNET_PRIME, s2)
    return s0


def poseidon_hash(x: int, y: int) -> int:
    """poseidonHash(x, y): one permutation of (x, y, 2)."""
    return hades_permutation(int(x) % STARKNET_PRIME, int(y) % STARKNET_PRIME, 2)[0]


def construct_felt252_from_m31s(word) -> int:
    """vcs/poseidon252_merkle.ts:86-122: 8 M31 values, 31 bits each, the first most significant."""
    if len(word) != ELEMENTS_IN_BLOCK:
        raise ValueError(f"Expected exactly 8 M31 elements, got {len(word)}")
    acc = 0
    for m in word:
        acc = (acc << 31) | int(m.value if isinstance(m, M31) else m)
    return acc


class Poseidon252MerkleHasher:
    """vcs/poseidon252_merkle.ts:19-73: hashNode on the host (the verifier's handful of nodes)."""

    @staticmethod
    def hashNode(children, column_values) -> FieldElement252:
        values = []
        if children is not None:
            values += [children[0].toBigInt(), children[1].toBigInt()]
        cols = list(column_values)
        n_blocks = -(-len(cols) // ELEMENTS_IN_BLOCK)
        cols += [0] * (ELEMENTS_IN_BLOCK * n_blocks - len(cols))
        for i in range(0, len(cols), ELEMENTS_IN_BLOCK):
            values.append(construct_felt252_from_m31s(cols[i:i + ELEMENTS_IN_BLOCK]))
        return FieldElement252.from_(poseidon_hash_many(values))

    hash_node = hashNode


class Poseidon252Channel:
    """channel/poseidon.ts:122-360, with the reference's surface and error texts.  Channel time follows the reference:
    mixing counts a challenge and resets n_sent; every draw counts one sent hash."""
    BYTES_PER_HASH = BYTES_PER_FELT252

    def __init__(self, digest: FieldElement252 | None = None, n_challenges: int = 0, n_sent: int = 0):
        self._felt = digest if digest is not None else FieldElement252.zero()
        self.n_challenges, self.n_sent = n_challenges, n_sent

    create = classmethod(lambda cls: cls())

    @classmethod
    def fromState(cls, digest: FieldElement252, n_challenges: int, n_sent: int) -> "Poseidon252Channel":
        return cls(digest, n_challenges, n_sent)

    def clone(self) -> "Poseidon252Channel":
        return Poseidon252Channel(self._felt, self.n_challenges, self.n_sent)

    def digest(self) -> FieldElement252:
        return self._felt

    def getChannelTime(self) -> tuple:
        return (self.n_challenges, self.n_sent)

    def update_digest(self, d: FieldElement252) -> None:
        self._felt = d
        self.n_challenges += 1
        self.n_sent = 0

    updateDigest = update_digest

    def _draw_felt252(self) -> FieldElement252:
        res = FieldElement252.from_(poseidon_hash(self._felt.toBigInt(), self.n_sent))
        self.n_sent += 1
        return res

    def _draw_base_felts(self) -> list:
        cur = self._draw_felt252().toBigInt()
        out = []
        for _ in range(FELTS_PER_HASH):
            out.append(M31.reduce(cur & (2**31 - 1)))
            cur >>= 31
        return out

    def trailing_zeros(self) -> int:
        """channel/poseidon.ts:209-229: the first 16 bytes of the big-endian encoding read as a little-endian u128 — so the count
        starts at bit 248 of the digest (a reference quirk kept as is)."""
        v = int.from_bytes(self._felt.toBytesBe()[:16], "little")
        return 128 if v == 0 else (v & -v).bit_length() - 1

    def mix_felts(self, felts, _le_bytes: bytes | None = None) -> None:
        """channel/poseidon.ts:231-255: two QM31 per element, M31 words base 2^31."""
        res = [self._felt.toBigInt()]
        for i in range(0, len(felts), 2):
            acc = 0
            for f in felts[i:i + 2]:
                for m in f.tup():
                    acc = (acc * 2**31 + int(m)) % STARKNET_PRIME
            res.append(acc)
        self.update_digest(FieldElement252.from_(poseidon_hash_many(res)))

    def mix_u32s(self, data) -> None:
        """channel/poseidon.ts:257-292: padded to a multiple of 7 words, 7 words base 2^32 (big-endian) per element."""
        data = list(data)
        for i, w in enumerate(data):
            if not (isinstance(w, (int, np.integer)) and 0 <= int(w) <= _MAX_U32):
                raise TypeError(f"Invalid u32 value at index {i}: {w}")
        data = [int(w) for w in data] + [0] * (6 - (len(data) + 6) % 7)
        felts = []
        for i in range(0, len(data), 7):
            acc = 0
            for w in data[i:i + 7]:
                acc = (acc * 2**32 + w) % STARKNET_PRIME
            felts.append(acc)
        self.update_digest(FieldElement252.from_(poseidon_hash_many([self._felt.toBigInt()] + felts)))

    def mix_u64(self, value: int) -> None:
        """channel/poseidon.ts:294-307."""
        if not (isinstance(value, (int, np.integer)) and 0 <= int(value) < 2**64):
            raise TypeError(f"Invalid u64 value: {value}")
        value = int(value)
        self.mix_u32s([0, 0, 0, 0, 0, (value >> 32) & _MAX_U32, value & _MAX_U32])

    def mix_root(self, root: FieldElement252) -> None:
        """Poseidon252MerkleChannel.mix_root on this channel (so that callers written against a channel's mix_root work)."""
        Poseidon252MerkleChannel.mix_root(self, root)

    def draw_felt(self):
        from .fields import QM31
        f = self._draw_base_felts()
        return QM31.from_u32_unchecked(*[m.value for m in f[:SECURE_EXTENSION_DEGREE]])

    def draw_felts(self, n_felts: int) -> list:
        from .fields import QM31
        if not isinstance(n_felts, int) or n_felts < 0:
            raise TypeError("n_felts must be a non-negative integer")
        out, buf = [], []
        while len(out) < n_felts:
            if len(buf) < SECURE_EXTENSION_DEGREE:
                buf += self._draw_base_felts()
            out.append(QM31.from_u32_unchecked(*[m.value for m in buf[:4]]))
            del buf[:4]
        return out

    def draw_random_bytes(self) -> bytes:
        """channel/poseidon.ts:339-356: 31 bytes, least significant first."""
        cur = self._draw_felt252().toBigInt()
        return bytes((cur >> (8 * i)) & 0xFF for i in range(BYTES_PER_FELT252))


class Poseidon252MerkleChannel:
    """vcs/poseidon252_merkle.ts:146-178 (+ what the prover and verifier need to pick this channel's trees)."""

    @staticmethod
    def mix_root(channel, root: FieldElement252) -> None:
        if not isinstance(channel, Poseidon252Channel):
            raise TypeError("Expected Poseidon252Channel")
        channel.update_digest(FieldElement252.from_(poseidon_hash_many([channel.digest().toBigInt(), root.toBigInt()])))

    mixRoot = mix_root
    # hasher / prover of this channel's trees: set below (Poseidon252MerkleProver is defined further down)
    hasher = Poseidon252MerkleHasher


class DevicePoseidon252Channel:
    """The Poseidon252Channel's state (digest limbs, n_challenges, n_sent) mirrored in 40 bytes of device memory — the surface of
    channel.DeviceChannel — so that a launch sequence (FRI commit: tree -> mix_root -> draw_felt -> fold -> tree ...) never waits
    for the host (csrc/poseidon_coop.hip: one wave, the permutation spread over 8 lanes)."""

    def __init__(self, host: Poseidon252Channel, buf=None):
        self.buf = buf if buf is not None else L.DeviceBuffer(64)
        self.load(host)

    def load(self, host: Poseidon252Channel, tail=None) -> None:
        """(Re)start from the host channel's state (one 64-byte upload).  tail: words the owner of a larger buffer keeps behind the
        16 state words, sent in the same upload."""
        if not isinstance(host, Poseidon252Channel):
            raise TypeError("Expected Poseidon252Channel")
        self.host = host
        st = np.zeros(16 + (0 if tail is None else len(tail)), dtype=np.uint32)
        if tail is not None:
            st[16:] = tail
        st[:8] = host.digest().to_words()
        st[8], st[9] = host.n_challenges, host.n_sent
        self.buf.upload(st)

    def mix_root_draw_felt(self, root_ptr: int | None, felt_ptr: int | None) -> None:
        """mix_root of the element at device address root_ptr, then draw_felt into the 4 words at felt_ptr (either may be None)."""
        L.call("tstwo_poseidon252_channel_mix_root_draw_felt", C.c_void_p(self.buf.ptr), C.c_void_p(root_ptr or 0), C.c_void_p(felt_ptr or 0))

    def sync_to_host(self, st=None) -> Poseidon252Channel:
        """The host channel continues from the device state (st: the 10 state words when the caller already fetched them)."""
        if st is None:
            st = self.buf.download(count=10)
        self.host._felt = FieldElement252.from_words(st[:8])
        self.host.n_challenges, self.host.n_sent = int(st[8]), int(st[9])
        return self.host


# ---- device trees
class FeltSlices(_LazyList):
    """FieldElement252 values over one bytes object of 32-byte little-endian limb records (a hash witness from the device)."""
    __slots__ = ("raw", "n")

    def __init__(self, raw: bytes, n: int):
        self.raw, self.n, self._items = raw, n, None

    def _n(self): return self.n
    def _make(self, i): return FieldElement252.from_le_bytes(self.raw[32 * i:32 * i + 32])


class DeviceFeltLayer(DeviceHashLayer):
    """A layer of FieldElement252 in device memory (8 limbs each)."""

    def toCpu(self) -> list: return [FieldElement252.from_le_bytes(bytes(r)) for r in self.to_numpy()]
    def at(self, i: int) -> FieldElement252: return FieldElement252.from_le_bytes(super().at(i))


class HipPoseidon252MerkleOps:
    """MerkleOps<FieldElement252>.commitOnLayer (backend/cpu/poseidon252.ts:44-78) on the GPU."""

    @staticmethod
    def commitOnLayer(logSize: int, prevLayer: DeviceHashLayer | None, columns) -> DeviceFeltLayer:
        n = 1 << logSize
        for c in columns:
            if c.len() != n:
                raise ValueError("column length does not match the layer size")
        if prevLayer is not None and len(prevLayer) != 2 * n:
            raise ValueError("previous layer must have twice the nodes")
        out = DeviceFeltLayer(L.DeviceBuffer(32 * n), n)
        L.call("tstwo_poseidon252_merkle_commit_layer", logSize, _vp(prevLayer.ptr if prevLayer is not None else 0),
               L.ptr_array([c.ptr for c in columns]), len(columns), _vp(out.ptr))
        return out

    @staticmethod
    def hash_many(messages) -> list:
        """poseidonHashMany of equally long messages (lists of FieldElement252 / ints) on the device."""
        messages = [list(m) for m in messages]
        if not messages:
            return []
        k = len(messages[0])
        if any(len(m) != k for m in messages):
            raise ValueError("messages must have the same length")
        words = np.array([[w for x in m for w in FieldElement252.from_(int(x)).to_words()] for m in messages], dtype=np.uint32)
        src = L.DeviceBuffer(max(words.nbytes, 32))
        dst = L.DeviceBuffer(32 * len(messages))
        if words.nbytes:
            src.upload(words.reshape(-1))
        L.call("tstwo_poseidon252_hash_many", _vp(src.ptr), len(messages), k, _vp(dst.ptr))
        out = dst.download(np.uint32).reshape(-1, 8)
        return [FieldElement252.from_words(r) for r in out.tolist()]


class Poseidon252MerkleProver(MerkleProver):
    """MerkleProver over Poseidon252 (vcs/prover.ts with MerkleOps<FieldElement252>): the root and the hash witnesses are
    FieldElement252.  Same layout as the Blake2s prover, so decommit / decommit_many are inherited."""

    _hash_of = staticmethod(FieldElement252.from_le_bytes)
    _hashes_of = FeltSlices
    _commit_entry = "tstwo_poseidon252_merkle_commit"

    @staticmethod
    def commit_many(column_sets, sync_root: bool = True) -> list:
        """One tree after the other (each is one launch sequence; the trees are VALU-bound, not latency-bound)."""
        return [Poseidon252MerkleProver.commit(list(cs), sync_root=sync_root) for cs in column_sets]


Poseidon252MerkleChannel.prover = Poseidon252MerkleProver


def grind_poseidon252(channel: Poseidon252Channel, pow_bits: int, start_nonce: int = 0) -> int:
    """GrindOps over Poseidon252Channel (backend/cpu/grind.ts:31-42) on the GPU: the first nonce the sequential loop finds."""
    L.ensure_init()
    d = np.array(channel.digest().to_words(), dtype=np.uint32)
    out = C.c_uint64(0)
    L.call("tstwo_grind_poseidon252", d.ctypes.data_as(L.u32p), int(pow_bits), int(start_nonce), C.byref(out))
    return out.value
