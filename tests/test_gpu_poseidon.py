"""Poseidon252 Merkle channel on the MI355X: hash_many, commitOnLayer, whole trees, decommitment through the Blake2s gather
entries, grind and the commitment scheme, every output word for word against the independent model (tests/poseidon_model.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import poseidon_model as M
import tstwo_amd as T
from tstwo_amd import _lib as L
from tstwo_amd.poseidon import FieldElement252, HipPoseidon252MerkleOps, Poseidon252MerkleProver, grind_poseidon252
from tstwo_amd.vcs import MerkleVerifier

pytestmark = pytest.mark.gpu

M31_P = 2**31 - 1
EDGE = [0, 1, M.P - 1, M.P - 2, 2**251, 2**192, 2**192 - 1, 2**128 - 1, 2**64 - 1, 2**32 - 1, M.P - 2**192]


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


class ModelHasher:
    """hashNode of the model, shaped for MerkleVerifier (children and root as FieldElement252)."""

    @staticmethod
    def hashNode(children, vals):
        ch = None if children is None else (int(children[0]), int(children[1]))
        return FieldElement252(M.hash_node(ch, [int(v.value if hasattr(v, "value") else v) for v in vals]))


def rand_cols(rng, n_cols, log):
    return [rng.integers(0, M31_P, size=1 << log, dtype=np.uint32) for _ in range(n_cols)]


def hip_cols(cols):
    return [T.HipColumn(c) for c in cols]


def layer_words(tree, lg):
    return tree.layers[lg].to_numpy().view("<u4").reshape(-1, 8)


def felt_of(words):
    return M.from_words([int(w) for w in words])


# ---------------------------------------------------------------- hash_many
@pytest.mark.parametrize("k", range(1, 8))
def test_hash_many_matches_model(k):
    rng = np.random.default_rng(100 + k)
    n = 96
    msgs = []
    for i in range(n):
        m = []
        for j in range(k):
            if (i + j) % 3 == 0:
                m.append(EDGE[(i * 7 + j) % len(EDGE)])
            else:
                m.append(int.from_bytes(rng.bytes(32), "little") % M.P)
        msgs.append(m)
    got = HipPoseidon252MerkleOps.hash_many(msgs)
    for m, g in zip(msgs, got):
        assert g.toBigInt() == M.hash_many(m)


def test_hash_many_raw_abi_words():
    """The C entry itself: 8 little-endian limbs in, 8 out."""
    msgs = [[M.P - 1, 5], [0, 0], [2**251, 1]]
    words = np.array([[w for x in m for w in M.to_words(x)] for m in msgs], dtype=np.uint32).reshape(-1)
    src, dst = L.DeviceBuffer(words.nbytes), L.DeviceBuffer(32 * len(msgs))
    src.upload(words)
    L.call("tstwo_poseidon252_hash_many", C.c_void_p(src.ptr), len(msgs), 2, C.c_void_p(dst.ptr))
    out = dst.download(np.uint32).reshape(-1, 8)
    assert [felt_of(r) for r in out] == [M.hash_many(m) for m in msgs]


# ---------------------------------------------------------------- commit_layer / commit
SHAPES = [(0, 0), (1, 0), (3, 1), (8, 3), (9, 4), (20, 0), (32, 10)]


@pytest.mark.parametrize("n_cols,log", SHAPES)
def test_commit_layer_and_tree_match_model(n_cols, log):
    rng = np.random.default_rng(1000 + 37 * n_cols + log)
    cols = rand_cols(rng, n_cols, log)
    if cols:
        cols[0][0] = M31_P - 1                  # the largest M31 value
    expect = M.commit([c.tolist() for c in cols]) if n_cols else [[M.hash_node(None, [])]]
    tree = Poseidon252MerkleProver.commit(hip_cols(cols))
    assert tree.root().toBigInt() == expect[0][0]
    for lg in range(len(expect)):
        assert [felt_of(r) for r in layer_words(tree, lg)] == expect[lg], lg
    # commitOnLayer by layer, through the ops
    hc = hip_cols(cols)
    prev = None
    for lg in range(log, -1, -1):
        prev = HipPoseidon252MerkleOps.commitOnLayer(lg, prev, hc if lg == log else [])
        assert [x.toBigInt() for x in prev.toCpu()] == expect[lg]


def test_commit_mixed_sizes_match_model():
    rng = np.random.default_rng(77)
    logs = [3, 11, 7, 11, 5, 9, 3, 8, 11, 6]
    cols = [rng.integers(0, M31_P, size=1 << lg, dtype=np.uint32) for lg in logs]
    expect = M.commit([c.tolist() for c in cols])
    tree = Poseidon252MerkleProver.commit(hip_cols(cols))
    for lg in range(12):
        assert [felt_of(r) for r in layer_words(tree, lg)] == expect[lg], lg


def test_many_columns_in_one_layer():
    """More columns at one layer than travel in the kernel argument (device pointer table)."""
    rng = np.random.default_rng(78)
    cols = rand_cols(rng, 70, 2)
    expect = M.commit([c.tolist() for c in cols])
    tree = Poseidon252MerkleProver.commit(hip_cols(cols))
    assert tree.root().toBigInt() == expect[0][0]


# ---------------------------------------------------------------- decommitment on a Poseidon tree
def test_decommit_through_gather_entries_matches_host_walk_and_verifies():
    rng = np.random.default_rng(91)
    logs = [6, 6, 4, 6, 5, 3, 4, 6, 2]
    cols = [rng.integers(0, M31_P, size=1 << lg, dtype=np.uint32) for lg in logs]
    hc = hip_cols(cols)
    tree = Poseidon252MerkleProver.commit(hc)
    queries = {6: [1, 7, 40, 63], 4: [3, 9], 2: [0]}
    vals, dec = tree.decommit(queries, hc)
    wvals, wdec = tree._decommit_walk(queries, hc)
    assert list(vals) == list(wvals)
    assert list(dec.hashWitness) == list(wdec.hashWitness)
    assert list(dec.columnWitness) == list(wdec.columnWitness)
    assert all(isinstance(h, FieldElement252) for h in dec.hashWitness)
    mq, mh, mw = M.decommit(M.commit([c.tolist() for c in cols]), [c.tolist() for c in cols], queries)
    assert [v.value for v in vals] == mq and [h.toBigInt() for h in dec.hashWitness] == mh and [v.value for v in dec.columnWitness] == mw
    MerkleVerifier(ModelHasher, tree.root(), logs).verify(queries, vals, dec)
    MerkleVerifier(T.Poseidon252MerkleHasher, tree.root(), logs).verify(queries, vals, dec)
    bad = copy.deepcopy(dec)
    bad.hashWitness[0] = FieldElement252((bad.hashWitness[0].toBigInt() + 1) % M.P)
    with pytest.raises(ValueError, match="Root mismatch"):
        MerkleVerifier(T.Poseidon252MerkleHasher, tree.root(), logs).verify(queries, vals, bad)


@pytest.mark.parametrize("log", [20, 22])
def test_large_tree_sampled_against_model(log):
    rng = np.random.default_rng(5000 + log)
    cols = rand_cols(rng, 32, log)
    hc = hip_cols(cols)
    tree = Poseidon252MerkleProver.commit(hc)
    prev = None
    for lg in range(log, -1, -1):
        words = layer_words(tree, lg)
        idx = sorted(set(rng.integers(0, 1 << lg, size=min(256, 1 << lg)).tolist()))
        for i in idx:
            children = None if lg == log else (felt_of(prev[2 * i]), felt_of(prev[2 * i + 1]))
            vals = [int(c[i]) for c in cols] if lg == log else []
            assert felt_of(words[i]) == M.hash_node(children, vals), (lg, i)
        prev = words
    queries = {log: sorted(set(rng.integers(0, 1 << log, size=128).tolist()))}
    vals, dec = tree.decommit(queries, hc)
    MerkleVerifier(ModelHasher, tree.root(), [log] * 32).verify(queries, vals, dec)


# ---------------------------------------------------------------- grind
@pytest.mark.parametrize("pow_bits", [0, 1, 2, 3, 8, 12, 16])
def test_grind_matches_sequential_loop(pow_bits):
    digests = [0, M.P - 1, M.hash_many([pow_bits, 7])] if pow_bits < 16 else [M.hash_many([16, 1])]
    for d in digests:
        for start in ([0, 1000] if pow_bits < 16 else [5]):
            out = C.c_uint64(0)
            dw = np.array(M.to_words(d), dtype=np.uint32)
            L.call("tstwo_grind_poseidon252", dw.ctypes.data_as(L.u32p), pow_bits, start, C.byref(out))
            assert out.value == M.grind(d, pow_bits, start), (d, pow_bits, start)


def test_grind_dispatches_on_the_channel():
    ch = T.Poseidon252Channel()
    ch.mix_u64(42)
    n = T.grind(ch, 9)
    assert n == M.grind(ch.digest().toBigInt(), 9)
    assert grind_poseidon252(ch, 9) == n
    c2 = ch.clone()
    c2.mix_u64(n)
    assert c2.trailing_zeros() >= 9


def test_grind_rejects_a_non_canonical_digest():
    out = C.c_uint64(0)
    dw = np.array(M.to_words(M.P), dtype=np.uint32)
    with pytest.raises(L.TstwoError, match="canonical"):
        L.call("tstwo_grind_poseidon252", dw.ctypes.data_as(L.u32p), 1, 0, C.byref(out))


# ---------------------------------------------------------------- FRI and the commitment scheme over Poseidon252
def _secure_low_degree_eval(log_deg, log_blowup, seed):
    domain = T.CanonicCoset(log_deg + log_blowup).circleDomain()
    tw = T.precompute_twiddles(domain.halfCoset)
    rng = np.random.default_rng(seed)
    polys = [T.HipCirclePoly(T.HipColumn(rng.integers(0, M31_P, size=1 << log_deg, dtype=np.uint32))) for _ in range(4)]
    evs = T.evaluate_polynomials(polys, domain, tw)
    return T.SecureEvaluation(domain, T.SecureColumnByCoords([e.values for e in evs])), tw


def test_fri_round_trip_over_poseidon():
    cfg = T.FriConfig(2, 2, 10)
    col, tw = _secure_low_degree_eval(7, 2, 600)
    ch = T.Poseidon252Channel()
    prover = T.FriProver.commit(ch, cfg, [col], tw, merkle_channel=T.Poseidon252MerkleChannel)
    # every layer's tree is the model's tree of the same columns
    first_cols = [c.to_numpy().tolist() for c in col.values.columns]
    assert prover.first_layer.merkle_tree.root().toBigInt() == M.commit(first_cols)[0][0]
    for layer in prover.inner_layers:
        lc = [c.to_numpy().tolist() for c in layer.evaluation.values.columns]
        assert layer.merkle_tree.root().toBigInt() == M.commit(lc)[0][0]
    proof, positions = prover.decommit(ch)
    assert isinstance(proof.first_layer.commitment, FieldElement252)
    vch = T.Poseidon252Channel()
    v = T.FriVerifier.commit(vch, cfg, proof, [T.CirclePolyDegreeBound(7)], merkle_channel=T.Poseidon252MerkleChannel)
    assert v.sample_query_positions(vch) == positions
    v.decommit([col.values.gather(positions[col.domain.logSize()])])
    assert vch.digest() == ch.digest()


def _pcs(config, logs, seed):
    blow = config.fri_config.log_blowup_factor
    max_log = max(lg for t in logs for lg in t)
    tw = T.precompute_twiddles(T.CanonicCoset(max_log + blow).circleDomain().halfCoset)
    scheme = T.CommitmentSchemeProver(config, tw, merkle_channel=T.Poseidon252MerkleChannel)
    ch = T.Poseidon252Channel()
    config.mix_into(ch)
    rng = np.random.default_rng(seed)
    for t in logs:
        tb = scheme.tree_builder()
        tb.extend_evals([T.HipCircleEvaluation(T.CanonicCoset(lg).circleDomain(), T.HipColumn(rng.integers(0, M31_P, size=1 << lg, dtype=np.uint32)))
                         for lg in t])
        tb.commit(ch)
    return scheme, ch


def test_commitment_scheme_over_poseidon_proves_and_verifies():
    config = T.PcsConfig(pow_bits=10, fri_config=T.FriConfig(1, 1, 6))
    logs = [[6, 6, 5], [6, 4]]
    scheme, ch = _pcs(config, logs, 3000)
    for t in scheme.trees:
        assert t.commitment.root().toBigInt() == M.commit([ev.values.to_numpy().tolist() for ev in t.evaluations])[0][0]
    point = T.CirclePoint.get_random_point(ch)
    pts = [[[point]] * 3, [[point]] * 2]
    proof = scheme.prove_values(pts, ch)
    assert all(isinstance(c, FieldElement252) for c in proof.commitments)
    assert isinstance(proof.fri_proof.first_layer.commitment, FieldElement252)

    def verify(pr):
        v = T.CommitmentSchemeVerifier(config, T.Poseidon252MerkleChannel)
        vch = T.Poseidon252Channel()
        config.mix_into(vch)
        for t, root in zip(logs, pr.commitments):
            v.commit(root, t, vch)
        vp = T.CirclePoint.get_random_point(vch)
        v.verify_values([[[vp]] * 3, [[vp]] * 2], pr, vch)
        return vch
    assert verify(proof).digest() == ch.digest()
    bad = copy.deepcopy(proof)
    bad.queried_values[0][0] = bad.queried_values[0][0].add(T.M31.one())
    with pytest.raises(T.VerificationError, match="Merkle verification failed"):
        verify(bad)
    bad = copy.deepcopy(proof)
    bad.decommitments[1].hashWitness[0] = FieldElement252((bad.decommitments[1].hashWitness[0].toBigInt() + 1) % M.P)
    with pytest.raises(T.VerificationError, match="Merkle verification failed"):
        verify(bad)
    bad = copy.deepcopy(proof)
    bad.proof_of_work += 1
    with pytest.raises((T.VerificationError, T.FriVerificationError)):
        verify(bad)
