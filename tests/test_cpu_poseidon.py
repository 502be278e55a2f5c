"""Poseidon252 Merkle channel on the host: the independent model (tests/poseidon_model.py) against the reference's known-answer
values, the library's compiled round-constant table against the model, and the host classes of tstwo_amd against the model."""
import copy
import os
import re
import subprocess
import sys

import pytest

import poseidon_model as M
from tstwo_amd import poseidon as PS
from tstwo_amd.fields import M31, QM31
from tstwo_amd.vcs import MerkleDecommitment, MerkleVerifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = os.path.join(ROOT, "tstwo_amd", "csrc", "poseidon_constants.h")


# ---------------------------------------------------------------- the model against the reference's known answers
def test_model_reproduces_the_reference_hash_node_values():
    """test/vcs/poseidon252_merkle.test.ts:10-34 (values from Rust)."""
    assert M.hash_node(None, [0, 1]) == 2552053700073128806553921687214114320458351061521275103654266875084493044716
    assert M.hash_node((1, 2), [3]) == 159358216886023795422515519110998391754567506678525778721401012606792642769


def test_model_reproduces_the_reference_channel_digest():
    """test/channel/poseidon.test.ts:312-318."""
    c = M.Channel()
    c.mix_u32s([1, 2, 3, 4, 5, 6, 7, 8, 9])
    assert c.digest == 0x078f5cf6a2e7362b75fc1f94daeae7ebddd64e6b2db771717519af7193dfa80b


# ---------------------------------------------------------------- the compiled table
def test_compiled_round_constants_equal_the_model():
    """poseidon_constants.h holds ARK * 2^256 mod p (Montgomery form) as 8 little-endian limbs per constant."""
    src = open(CONSTANTS).read()
    body = src[src.index("kArk["):]
    rows = re.findall(r"\{(0x[0-9a-f]{8}u(?:, 0x[0-9a-f]{8}u){7})\}", body)
    assert len(rows) == 3 * 91
    r_inv = pow(2**256, -1, M.P)
    got = [sum(int(w.rstrip("u"), 16) << (32 * k) for k, w in enumerate(r.split(", "))) * r_inv % M.P for r in rows]
    assert got == [M.ARK[i][j] for i in range(91) for j in range(3)]
    one = re.search(r"kOneMont\[8\] = \{([^}]*)\}", src).group(1)
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * k) for k, w in enumerate(one.split(","))) == 2**256 % M.P
    r2 = re.search(r"kR2\[8\] = \{([^}]*)\}", src).group(1)
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * k) for k, w in enumerate(r2.split(","))) == 2**512 % M.P


def test_constant_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_poseidon_constants.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------- host classes against the model
def test_host_hash_many_and_hasher_match_the_model():
    vals = [0, 1, M.P - 1, 2**251, 12345, 2**192]
    for k in range(0, 7):
        assert PS.poseidon_hash_many(vals[:k]) == M.hash_many(vals[:k])
    assert PS.poseidon_hash(3, 4) == M.hash2(3, 4)
    for children in (None, (PS.FieldElement252(5), PS.FieldElement252(M.P - 1))):
        for n in (0, 1, 7, 8, 9, 17):
            cols = [(i * 2654435761) % (2**31 - 1) for i in range(n)]
            got = PS.Poseidon252MerkleHasher.hashNode(children, [M31(c) for c in cols])
            ch = None if children is None else tuple(int(c) for c in children)
            assert got.toBigInt() == M.hash_node(ch, cols)


def test_field_element_conversions():
    x = PS.FieldElement252.from_(M.P + 5)
    assert x.toBigInt() == 5 and getattr(PS.FieldElement252, "from")(7).toBigInt() == 7
    y = PS.FieldElement252(2**251 + 3)
    assert PS.FieldElement252.from_words(y.to_words()) == y and y.to_words() == M.to_words(2**251 + 3)
    assert PS.FieldElement252.from_le_bytes(y.to_le_bytes()) == y
    assert y.toBytesBe() == (2**251 + 3).to_bytes(32, "big")
    assert PS.FieldElement252.fromHexBe("0x10").toBigInt() == 16 and PS.FieldElement252.fromHexBe("zz") is None
    with pytest.raises(TypeError, match="Value must be in range"):
        PS.FieldElement252(M.P)
    with pytest.raises(ValueError, match="Division by zero"):
        y.floorDiv(PS.FieldElement252.zero())


def _qm(i):
    return QM31.from_u32_unchecked(i % (2**31 - 1), (3 * i) % (2**31 - 1), (7 * i + 1) % (2**31 - 1), 2**31 - 2)


def test_channel_matches_the_model_method_by_method():
    c, m = PS.Poseidon252Channel(), M.Channel()
    c.mix_u32s(list(range(1, 10)))
    m.mix_u32s(list(range(1, 10)))
    assert c.digest().toBigInt() == m.digest == 0x078f5cf6a2e7362b75fc1f94daeae7ebddd64e6b2db771717519af7193dfa80b
    for n in (0, 1, 2**32, 2**64 - 1):
        c.mix_u64(n)
        m.mix_u64(n)
        assert c.digest().toBigInt() == m.digest
    for k in (0, 1, 2, 3, 5):
        felts = [_qm(i + k) for i in range(k)]
        c.mix_felts(felts)
        m.mix_felts([f.tup() for f in felts])
        assert c.digest().toBigInt() == m.digest
    root = PS.FieldElement252(M.hash_many([9]))
    PS.Poseidon252MerkleChannel.mix_root(c, root)
    m.mix_root(root.toBigInt())
    assert c.digest().toBigInt() == m.digest
    c.mix_root(root)
    m.mix_root(root.toBigInt())
    assert c.digest().toBigInt() == m.digest
    assert c.draw_felt().tup() == m.draw_felt()
    assert [f.tup() for f in c.draw_felts(5)] == m.draw_felts(5)
    assert c.draw_random_bytes() == m.draw_random_bytes()
    assert (c.n_challenges, c.n_sent) == (m.n_challenges, m.n_sent)
    assert c.trailing_zeros() == m.trailing_zeros()
    e = c.clone()
    assert e.digest() == c.digest() and e.getChannelTime() == c.getChannelTime()


def test_channel_time_and_errors_follow_the_reference():
    """channel/poseidon.ts test_channel_time (Rust text): a random-bytes draw and 9 felts send 1 + 5 hashes, no challenge."""
    c = PS.Poseidon252Channel.create()
    c.draw_random_bytes()
    assert (c.n_challenges, c.n_sent) == (0, 1)
    c.draw_felts(9)
    assert (c.n_challenges, c.n_sent) == (0, 6)
    c.mix_u64(1)
    assert (c.n_challenges, c.n_sent) == (1, 0)
    a, b = PS.Poseidon252Channel(), PS.Poseidon252Channel()
    a.mix_u64(0x1111222233334444)
    b.mix_u32s([0, 0, 0, 0, 0, 0x11112222, 0x33334444])
    assert a.digest() == b.digest()
    with pytest.raises(TypeError, match="Invalid u32 value at index 1"):
        c.mix_u32s([1, 2**32])
    with pytest.raises(TypeError, match="Invalid u64 value"):
        c.mix_u64(-1)
    with pytest.raises(TypeError, match="n_felts must be a non-negative integer"):
        c.draw_felts(-1)
    with pytest.raises(TypeError, match="Expected Poseidon252Channel"):
        PS.Poseidon252MerkleChannel.mix_root(object(), PS.FieldElement252(1))


def test_trailing_zeros_starts_at_bit_248():
    """The reference quirk: the count starts at bit 248 of the element, byte by byte upward in the big-endian encoding."""
    for v, tz in [(0, 128), (1 << 248, 0), (1 << 250, 2), (1 << 240, 8), (1 << 247, 15), (1, 128), (1 << 120, 128), (1 << 128, 120)]:
        assert PS.Poseidon252Channel(PS.FieldElement252(v)).trailing_zeros() == M.trailing_zeros(v) == tz, hex(v)


def test_merkle_verifier_accepts_a_model_tree_and_rejects_tampering():
    cols = [[(7 * i + 3 * c) % (2**31 - 1) for i in range(1 << lg)] for c, lg in enumerate([4, 4, 3, 2, 4, 1, 3, 4, 4, 4])]
    logs = [len(c).bit_length() - 1 for c in cols]
    layers = M.commit(cols)
    queries = {4: [2, 11], 3: [5], 1: [0]}
    q, h, w = M.decommit(layers, cols, queries)
    root = PS.FieldElement252(layers[0][0])
    dec = MerkleDecommitment([PS.FieldElement252(x) for x in h], [M31(x) for x in w])
    vals = [M31(x) for x in q]
    v = MerkleVerifier(PS.Poseidon252MerkleHasher, root, logs)
    v.verify(queries, vals, dec)
    bad = copy.deepcopy(dec)
    bad.hashWitness[0] = PS.FieldElement252((h[0] + 1) % M.P)
    with pytest.raises(ValueError, match="Root mismatch"):
        v.verify(queries, vals, bad)
    with pytest.raises(ValueError, match="Root mismatch"):
        v.verify(queries, [M31((vals[0].value + 1) % (2**31 - 1))] + vals[1:], dec)
    with pytest.raises(ValueError, match="Witness is too short"):
        v.verify(queries, vals, MerkleDecommitment(dec.hashWitness[:-1], dec.columnWitness))
    with pytest.raises(ValueError, match="Witness is too long"):
        v.verify(queries, vals, MerkleDecommitment(list(dec.hashWitness) + [root], dec.columnWitness))
