"""-m gpu: the LogUp-GKR range check inside a STARK (tstwo_amd/gkr_lookup.py gkr_range_check_stark_prove / _verify): the value
columns and the multiplicities are committed, the claims on the GKR input layers become mle_eval components, and the verifier
works from the proofs and the log sizes alone."""
import copy
import inspect

import numpy as np
import pytest

from tstwo_amd import _lib as L
from tstwo_amd import gkr_lookup as GL
from tstwo_amd.backend import HipColumn
from tstwo_amd.channel import Blake2sChannel
from tstwo_amd.fields import QM31
from tstwo_amd.gkr import GkrInputClaimMismatch
from tstwo_amd.gkr_verifier import GkrError, GkrMask
from tstwo_amd.logup import lookup_multiplicities
from tstwo_amd.pcs_verifier import VerificationError
from tstwo_amd.poseidon import Poseidon252Channel, Poseidon252MerkleChannel
from tstwo_amd.prover import InvalidLogupSum, StarkProof

pytestmark = pytest.mark.gpu

P = 2147483647


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def _values(n, k=2, seed=0):
    rng = np.random.default_rng(100 * n + seed)
    return [rng.integers(0, 1 << n, size=1 << n, dtype=np.uint32) for _ in range(k)]


def _prove(n, channel_cls=Blake2sChannel, merkle=None, values=None, **kw):
    cols = [HipColumn(v) for v in (values if values is not None else _values(n))]
    proof = GL.gkr_range_check_stark_prove(channel_cls(), n, cols, merkle=merkle, **kw)
    sizes = [n] * len(cols)
    del cols                                   # the verifier is never handed a value column: they are gone before it runs
    return proof, sizes


@pytest.mark.parametrize("n", [4, 8])
def test_prove_verify_blake2s(n):
    proof, sizes = _prove(n)
    assert len(proof.stark_proof.commitments) == 4
    assert [len(c) for c in proof.stark_proof.sampled_values[2]] == [3, 3, 3, 3, 2, 2, 2, 2]      # E at [-2, 0, 2], S at [-1, 0]
    GL.gkr_range_check_stark_verify(Blake2sChannel(), n, sizes, proof)


def test_prove_verify_poseidon252():
    proof, sizes = _prove(4, Poseidon252Channel, Poseidon252MerkleChannel)
    GL.gkr_range_check_stark_verify(Poseidon252Channel(), 4, sizes, proof, merkle=Poseidon252MerkleChannel)


def test_prove_verify_native():
    proof, sizes = _prove(4, native=True)
    GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, sizes, proof)


def test_the_verifier_signature_takes_no_column():
    params = list(inspect.signature(GL.gkr_range_check_stark_verify).parameters)
    assert params == ["channel", "log_range", "log_sizes", "proof", "config", "merkle"]
    assert not [p for p in params if "column" in p or "value" in p]


def test_an_out_of_range_value_fails_in_check_logup_sum(monkeypatch):
    n = 4
    values = _values(n)
    values[1][5] = 1 << n                                                       # one word outside [0, 2^n)
    mult = lookup_multiplicities(n, *[HipColumn(v) for v in values], order="natural", check=False)
    proof, sizes = _prove(n, values=values, multiplicities=mult)
    # the failure is the sum check's: nothing behind it runs
    from tstwo_amd import gkr as G
    seen = []
    real = G.check_logup_sum
    monkeypatch.setattr(GL, "check_logup_sum", lambda *a, **k: (seen.append(1), real(*a, **k)))
    monkeypatch.setattr(GL, "_stark_components", lambda *a, **k: pytest.fail("the verifier went past check_logup_sum"))
    with pytest.raises(InvalidLogupSum):
        GL.gkr_range_check_stark_verify(Blake2sChannel(), n, sizes, proof)
    assert seen == [1]


def _bump(v: QM31) -> QM31:
    t = list(v.tup())
    t[0] = (t[0] + 1) % P
    return QM31.from_u32_unchecked(*t)


@pytest.fixture(scope="module")
def honest():
    proof, sizes = _prove(4)
    GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, sizes, proof)
    return proof, sizes


REJECTED = (GkrError, InvalidLogupSum, GkrInputClaimMismatch, VerificationError, ValueError)


def test_a_changed_gkr_mask_word_is_rejected(honest):
    proof, sizes = honest
    for inst, layer in ((0, -1), (2, -1), (1, 0)):                              # the input layer's mask (the claim comes from it), an inner one
        bad = GL.GkrStarkProof(copy.deepcopy(proof.gkr_proof), proof.stark_proof)
        masks = bad.gkr_proof.layer_masks_by_instance[inst]
        cols = [list(c) for c in masks[layer].columns()]
        cols[1][0] = _bump(cols[1][0])                                          # one word of the denominators' mask
        masks[layer] = GkrMask(cols)
        with pytest.raises(REJECTED):
            GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, sizes, bad)


def test_a_changed_output_claim_is_rejected(honest):
    proof, sizes = honest
    bad = GL.GkrStarkProof(copy.deepcopy(proof.gkr_proof), proof.stark_proof)
    out = bad.gkr_proof.output_claims_by_instance[0]
    out[1] = _bump(out[1])
    with pytest.raises(REJECTED):
        GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, sizes, bad)


def test_a_changed_interaction_sample_is_rejected(honest):
    proof, sizes = honest
    stark = StarkProof(copy.deepcopy(proof.stark_proof.commitment_scheme_proof))
    stark.sampled_values[2][4][1] = _bump(stark.sampled_values[2][4][1])         # S, coordinate 0, at offset 0
    bad = GL.GkrStarkProof(proof.gkr_proof, stark)
    with pytest.raises(VerificationError):
        GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, sizes, bad)


def test_unequal_value_column_sizes_are_refused():
    with pytest.raises(ValueError, match="share one log size"):
        GL.gkr_range_check_stark_prove(Blake2sChannel(), 4, [HipColumn(np.zeros(16, dtype=np.uint32)), HipColumn(np.zeros(32, dtype=np.uint32))])


def test_two_log_sizes_in_one_proof():
    """Value columns of log size 5 against a table of log size 4: two mle_eval components, interaction columns of two sizes."""
    rng = np.random.default_rng(9)
    values = [rng.integers(0, 16, size=32, dtype=np.uint32) for _ in range(2)]
    proof = GL.gkr_range_check_stark_prove(Blake2sChannel(), 4, [HipColumn(v) for v in values])
    GL.gkr_range_check_stark_verify(Blake2sChannel(), 4, [5, 5], proof)
