"""The device channel's draw_felt (chan_mix_draw, csrc/blake2s.cuh) at the edges of its rejection rule, through every entry that
draws: tstwo_channel_mix_root_draw_felt, the tree hooks and the tail of tstwo_fri_commit_layers, and the GKR transcript kernels
(tstwo_gkr_round_finish[_dev], tstwo_gkr_layer_begin, tstwo_gkr_layer_end, tstwo_gkr_prove_batch).  The channel states come from
tests/golden/blake2s_draw_edges.json: searched on the CPU so that a chosen draw's first hash holds 2P or 2^32 - 1 (rejected: a
second hash is taken), 2P - 1 (accepted, reduces to P - 1) or P (reduces to 0).  Every output word is compared with the hashlib
model of tests/draw_edges.py; tests/test_cpu_draw_edges.py proves the fixtures and holds the lists below to the planted faults.

Not steered: the FOLD_COMMIT step of the FRI commit.  It occurs only above 2^9 rows with no column joining, so a trial would hash a
2^10-leaf tree (about 10^11 hashes for one fixture).  Its channel step is chan_step_from_lds, the function the FIRST_TREE and COMMIT
hooks run here."""
import ctypes as C
import struct

import numpy as np
import pytest

import draw_edges as D
import gkr_layer_model as LM
import gkr_model as M
import gkr_round_model as R
import sequence as SQ
from arena import SENTINEL, Arena, rin, rinout, rout

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402

FIX = D.load_fixtures()
CASE_LISTS = {entry: [c.name for c in D.CASES if c.entry == key] for entry, key in
              (("channel draw", "draw"), ("channel mix+draw", "mix"), ("fri commit", "fri"), ("gkr round_finish", "finish"),
               ("gkr layer_begin", "begin"), ("gkr layer_end", "end"), ("gkr prove_batch", "prove"))}
FORMS = ("draw only", "mix then draw", "mix only, then draw only")


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


def state_of(name):
    return np.array(FIX[name]["state"], dtype=np.uint32)


def words(a):
    return [int(w) for w in a]


def words_of(felts):
    return np.array([w for f in felts for w in f], dtype=np.uint32)


def steered(model, case):
    """the model took the number of hashes the case is about at the steered draw, and one everywhere else"""
    want = 2 if D.CONDITIONS[case.cond][2] else 1
    return [h for _, _, h in model.draws] == [want if i == case.target else 1 for i in range(len(model.draws))]


# ------------------------------------------------------------------ tstwo_channel_mix_root_draw_felt
@pytest.mark.parametrize("name", CASE_LISTS["channel draw"])
def test_channel_draw_only(name):
    case = D.BY_NAME[name]
    model, felt = D.run_model(case, FIX[name]["state"])
    assert steered(model, case)
    with Arena([rinout("chan", state_of(name)), rout("felt", 4)]) as A:
        L.call("tstwo_channel_mix_root_draw_felt", A.ptr("chan"), C.c_void_p(0), A.ptr("felt"))
        got = A.check()
    assert tuple(words(got["felt"])) == felt
    assert words(got["chan"]) == model.words()


@pytest.mark.parametrize("form", FORMS[1:])
@pytest.mark.parametrize("name", CASE_LISTS["channel mix+draw"])
def test_channel_mix_then_draw(name, form):
    case = D.BY_NAME[name]
    model, felt = D.run_model(case, FIX[name]["state"])
    assert steered(model, case)
    with Arena([rinout("chan", state_of(name)), rin("root", np.frombuffer(D.ROOT, dtype=np.uint8)), rout("felt", 4)]) as A:
        if form == "mix then draw":
            L.call("tstwo_channel_mix_root_draw_felt", A.ptr("chan"), A.ptr("root"), A.ptr("felt"))
        else:
            L.call("tstwo_channel_mix_root_draw_felt", A.ptr("chan"), A.ptr("root"), C.c_void_p(0))
            L.call("tstwo_channel_mix_root_draw_felt", A.ptr("chan"), C.c_void_p(0), A.ptr("felt"))
        got = A.check()
    assert tuple(words(got["felt"])) == felt
    assert words(got["chan"]) == model.words()


# ------------------------------------------------------------------ tstwo_fri_commit_layers
FRI_KINDS = {(3,): {"FIRST_TREE", "CIRCLE_WRITE", "TAIL"}, (4, 3): {"FIRST_TREE", "CIRCLE_WRITE", "COMMIT", "FOLD_LINE", "CIRCLE_ACCUM", "TAIL"}}
# which launch draws the steered alpha, by tests/fri_plan.py: the kind of the step that holds the channel step
FRI_DRAWN_BY = {((3,), 0): "FIRST_TREE", ((3,), 1): "TAIL", ((3,), 2): "TAIL", ((4, 3), 1): "COMMIT"}


def layers_bytes(log):
    return 32 * ((2 << log) - 1)


def fri_commit_device(col_logs, state):
    """tstwo_fri_commit_layers down to one row between guard bands: (channel words, alphas region, first tree, [(log, evaluation, tree)])"""
    from oracle import oracle as orc
    col_logs = list(col_logs)
    log = col_logs[0]
    tw_log = log + 1
    itw = orc.precompute_twiddles(orc.lib().orc_half_odds_initial(tw_log), tw_log)[1]
    n_trees = 1 + (log - 1)
    cap = n_trees + 3
    cols = D.fri_columns(col_logs)
    c_ = [f"col{j}_{k}" for j in range(len(col_logs)) for k in range(4)]
    regs = [rin(x, c) for x, c in zip(c_, [c for col in cols for c in col])]
    regs += [rin("itw", itw), rinout("chan", np.array(state, dtype=np.uint32)), rout("alphas", 4 * cap)]
    outs, n_out, first = (L.FriLayerOut * (n_trees + 1))(), C.c_size_t(0), L.vp()
    with Arena(regs) as A:
        L.call("tstwo_fri_commit_layers", A.ptrs(c_), L.u32x(col_logs), len(col_logs), A.ptr("itw"), tw_log, 0, A.ptr("chan"),
               A.ptr("alphas"), cap, C.byref(first), outs, n_trees + 1, C.byref(n_out))
        got = A.check()
        owned = [L.DeviceBuffer.adopt(first.value, layers_bytes(log))]
        layers = []
        for i in range(n_out.value):
            lg = outs[i].log_size
            ev = [L.DeviceBuffer.adopt(outs[i].cols[k], 4 << lg) for k in range(4)]
            tree = L.DeviceBuffer.adopt(outs[i].layers, layers_bytes(lg)) if outs[i].layers else None
            owned += ev + ([tree] if tree else [])
            layers.append((lg, [e.download() for e in ev], tree.download(np.uint8) if tree else None))
        first_tree = owned[0].download(np.uint8)
        for b in owned:
            b.free()
    return got["chan"], got["alphas"], first_tree, layers


@pytest.mark.parametrize("name", CASE_LISTS["fri commit"])
def test_fri_commit_layers(name):
    """Every tree, evaluation and alpha, the last layer and the channel against the per-layer loop on the CPU oracle and the model
    channel; the plan's kinds are asserted first, so that a change of the plan cannot silently move the draw to another launch."""
    import fri_plan
    case = D.BY_NAME[name]
    logs = tuple(case.spec)
    assert fri_plan.kinds(list(logs), 0) == FRI_KINDS[logs]
    drawn_by = [s.kind for s in fri_plan.plan(list(logs), 0)
                if s.kind != "TAIL" and s.alpha_out == case.target and s.kind in ("FIRST_TREE", "COMMIT", "FOLD_COMMIT")
                or s.kind == "TAIL" and s.alpha_out <= case.target < s.alpha_out + s.n_layers]
    assert drawn_by == [FRI_DRAWN_BY[(logs, case.target)]]
    model, first, mlayers, alphas = D.fri_commit_model(list(logs), FIX[name]["state"])
    assert steered(model, case) and len(alphas) == logs[0]
    chan, dalphas, dfirst, dlayers = fri_commit_device(logs, FIX[name]["state"])
    assert words(dalphas[:4 * len(alphas)]) == [w for a in alphas for w in a]
    assert (dalphas[4 * len(alphas):] == SENTINEL).all()
    assert dfirst.tobytes() == first.tobytes()
    assert [lg for lg, _, _ in dlayers] == [lg for lg, _, _ in mlayers]
    for (lg, dev_ev, dev_tree), (_, ev, tree) in zip(dlayers, mlayers):
        assert all((dev_ev[k] == ev[k]).all() for k in range(4)), lg
        assert (dev_tree is None) == (tree is None) and (tree is None or dev_tree.tobytes() == tree.tobytes()), lg
    assert words(chan) == model.words()


def _host_channel(state):
    import tstwo_amd as T
    ch = T.Blake2sChannel()
    ch._digest, ch.n_challenges, ch.n_sent = struct.pack("<8I", *state[:8]), int(state[8]), int(state[9])
    return ch


@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.entry == "fri" and c.target < 2])
def test_fri_prover_and_verifier_across_a_draw(name):
    """FriProver.commit (one library call, device channel) against its per-layer loop on the host channel, from the steered digest:
    roots, evaluations, last-layer coefficients and channel; then decommit, and FriVerifier from the same digest accepts.  The
    prover's last layer has two rows (FriConfig has no smaller one), so the transcript is the fixture's up to alpha 1 and the two
    alpha-2 cases of [3] do not exist in it: for those the oracle loop on the model channel (test_fri_commit_layers) stands alone.
    The host loop does not hand out its alphas; every evaluation below the first layer is a fold by them and is compared."""
    import tstwo_amd as T
    case, state = D.BY_NAME[name], FIX[name]["state"]
    cfg = T.FriConfig(0, 1, 3)
    logs = list(case.spec)
    tw = T.precompute_twiddles(T.CanonicCoset(logs[0]).circleDomain().halfCoset)

    def columns():
        return [T.SecureEvaluation(T.CanonicCoset(c).circleDomain(), T.SecureColumnByCoords([T.HipColumn(x) for x in col]))
                for c, col in zip(logs, D.fri_columns(logs))]
    cols = columns()
    ch, hch = _host_channel(state), _host_channel(state)
    prover = T.FriProver.commit(ch, cfg, cols, tw)
    host = T.FriProver.commit(hch, cfg, columns(), tw, device_channel=False)
    model = D.fri_commit_model(logs, state, last=1)
    assert steered(model[0], case)
    assert T.FriProver._device_capable(cols, tw), "the commit must take the device transcript"
    assert prover.first_layer.merkle_tree.root() == host.first_layer.merkle_tree.root() == model[1].reshape(-1)[:32].tobytes()
    assert len(prover.inner_layers) == len(host.inner_layers) == len(model[2]) - 1
    for la, lb, (lg, ev, tree) in zip(prover.inner_layers, host.inner_layers, model[2]):
        assert la.merkle_tree.root() == lb.merkle_tree.root() == tree.reshape(-1)[:32].tobytes(), lg
        for ca, cb, cm in zip(la.evaluation.values.to_numpy(), lb.evaluation.values.to_numpy(), ev):
            assert (ca == cb).all() and (ca == cm).all(), lg
    assert [c.tup() for c in prover.last_layer_poly.coeffs] == [c.tup() for c in host.last_layer_poly.coeffs]
    assert (ch.digest(), ch.n_challenges, ch.n_sent) == (hch.digest(), hch.n_challenges, hch.n_sent)
    proof, positions = prover.decommit(ch)
    vch = _host_channel(state)
    v = T.FriVerifier.commit(vch, cfg, proof, [T.CirclePolyDegreeBound(c - 1) for c in logs])
    assert v.sample_query_positions(vch) == positions
    v.decommit([c.values.gather(positions[c.domain.logSize()]) for c in cols])


# ------------------------------------------------------------------ tstwo_gkr_round_finish and its _dev twin
@pytest.mark.parametrize("dev", [False, True], ids=["by value", "dev"])
@pytest.mark.parametrize("name", CASE_LISTS["gkr round_finish"])
def test_gkr_round_finish(name, dev):
    case, state = D.BY_NAME[name], FIX[name]["state"]
    n = case.spec
    claims, corrs, rd = D.finish_inputs(n)
    model, (coeffs, ch, new_claims, new_corrs) = D.run_model(case, state)
    assert steered(model, case)
    sums = np.full(8 * n, SQ.SENTINEL, dtype=np.uint32)
    for i, (s, act) in enumerate(zip(rd["sums"], rd["active"])):
        if act:
            sums[8 * i:8 * i + 8] = words_of(s)
    regs = [rinout("chan", state_of(name), 4), rin("sums", sums), rinout("state", words_of([w for c, k in zip(claims, corrs) for w in (c, k)])),
            rout("poly", 20), rout("challenge", 4)]
    if dev:
        regs += [rin("y", words_of([rd["y"]])), rin("a", words_of([rd["a"]])), rin("alpha", words_of([rd["alpha"]])),
                 rinout("status", np.array([0], dtype=np.uint32), 4)]
    mask = sum(1 << i for i, a in enumerate(rd["active"]) if a)
    with Arena(regs) as A:
        if dev:
            L.call("tstwo_gkr_round_finish_dev", A.ptr("chan"), A.ptr("sums"), A.ptr("state"), n, C.c_uint64(mask), A.ptr("y"), A.ptr("a"),
                   A.ptr("alpha"), A.ptr("poly"), A.ptr("challenge"), A.ptr("status"))
        else:
            L.call("tstwo_gkr_round_finish", A.ptr("chan"), A.ptr("sums"), A.ptr("state"), n, C.c_uint64(mask), L.u32x(rd["y"]), L.u32x(rd["a"]),
                   L.u32x(rd["alpha"]), A.ptr("poly"), A.ptr("challenge"))
        got = A.check()
    assert words(got["poly"]) == [len(coeffs), 0, 0, 0] + [w for c in coeffs + [M.ZERO] * (4 - len(coeffs)) for w in c]
    assert tuple(words(got["challenge"])) == ch
    assert words(got["chan"]) == model.words()
    assert words(got["state"]) == words(words_of([w for c, k in zip(new_claims, new_corrs) for w in (c, k)]))
    assert not dev or int(got["status"][0]) == 0


# ------------------------------------------------------------------ tstwo_gkr_layer_begin / tstwo_gkr_layer_end
N_INST = 4


def lane_table(A, ln):
    t = (L.GkrLane * 1)()
    base = A.addr("cols")
    t[0].src = (L.vp * 8)(*[base + 12 * c for c in range(8)])
    t[0].out_src = (L.vp * 8)(*[base + 12 * (8 + c) for c in range(8)])
    t[0].inst, t[0].kind, t[0].shift, t[0].enter = ln["inst"], ln["kind"], ln["shift"], int(ln["enter"])
    return np.frombuffer(bytes(t), dtype=np.uint8)


def claim_words(claims):
    w = np.full(8 * N_INST, SQ.SENTINEL, dtype=np.uint32)
    for i, c in claims.items():
        w[8 * i:8 * i + 8] = words_of(list(c) + [M.ZERO] * (2 - len(c)))
    return w


@pytest.mark.parametrize("name", CASE_LISTS["gkr layer_begin"])
def test_gkr_layer_begin(name):
    """alpha then lambda: a rejection in the first draw moves the second to n_sent = 2, one in the second ends at n_sent = 3; an
    accepted edge word in either shows in the scalars"""
    case, state = D.BY_NAME[name], FIX[name]["state"]
    ln = D.lane_inputs(case.spec)
    model, ((alpha, lam, mstate, inv, v, bad), mclaims) = D.run_model(case, state)
    assert steered(model, case) and not bad and model.n_sent == 2 + D.CONDITIONS[case.cond][2]
    y = ln["y"]
    with Arena([rin("cols", ln["cols"].astype(np.uint32)), rinout("chan", state_of(name), 4), rin("claims", claim_words(ln["claims"])),
                rout("out_claims", 8 * N_INST), rout("state", 8), rout("scalars", 12), rin("y", words_of(y + [M.ZERO])),
                rout("inv", 4 * len(y)), rinout("status", np.array([0], dtype=np.uint32), 4),
                rinout("table", np.zeros(36, dtype=np.uint32))]) as A:
        table = lane_table(A, ln)
        A.buf.upload(table, A.layout.start["table"])
        L.call("tstwo_gkr_layer_begin", A.ptr("chan"), A.ptr("table"), 1, A.ptr("claims"), A.ptr("out_claims"), A.ptr("state"), A.ptr("scalars"),
               A.ptr("y"), len(y), A.ptr("inv"), A.ptr("status"))
        got = A.check()
    assert (got["table"].view(np.uint8) == table).all() and int(got["status"][0]) == 0
    assert words(got["chan"]) == model.words()
    assert tuple(words(got["scalars"][:4])) == alpha and tuple(words(got["scalars"][4:8])) == lam and tuple(words(got["scalars"][8:])) == v
    assert words(got["state"]) == words(words_of([w for s in mstate for w in s]))
    assert words(got["inv"]) == words(words_of(inv))
    assert (got["out_claims"] == claim_words({1: mclaims[1]} if ln["enter"] else {})).all()


@pytest.mark.parametrize("name", CASE_LISTS["gkr layer_end"])
def test_gkr_layer_end(name):
    """the grand-product mask is 2 felts (one block behind the digest), the LogUp mask 4 (two blocks)"""
    case, state = D.BY_NAME[name], FIX[name]["state"]
    ln = D.lane_inputs(case.spec)
    model, (ch, mask, mclaims) = D.run_model(case, state)
    assert steered(model, case) and len(model.mixes[0]) == (32 if case.spec == "gp" else 64)
    with Arena([rin("cols", ln["cols"].astype(np.uint32)), rinout("chan", state_of(name), 4), rout("masks", 16), rout("claims", 8 * N_INST),
                rout("challenge", 4), rinout("table", np.zeros(36, dtype=np.uint32))]) as A:
        table = lane_table(A, ln)
        A.buf.upload(table, A.layout.start["table"])
        L.call("tstwo_gkr_layer_end", A.ptr("chan"), A.ptr("table"), 1, A.ptr("masks"), A.ptr("claims"), A.ptr("challenge"))
        got = A.check()
    assert (got["table"].view(np.uint8) == table).all()
    assert words(got["chan"]) == model.words()
    assert tuple(words(got["challenge"])) == ch
    assert words(got["masks"]) == LM.mask_words(mask)
    assert (got["claims"] == claim_words({1: mclaims[1]})).all()


# ------------------------------------------------------------------ tstwo_gkr_prove_batch
@pytest.mark.parametrize("name", CASE_LISTS["gkr prove_batch"])
def test_gkr_prove_batch(name):
    """The whole proof of one call against the integer model on the model channel and against the host loop and the per-round
    device path; gkr_verifier accepts it from the same starting digest.  prove/begin0 cannot show a wrong draw (draw_edges.UNOBSERVABLE):
    it shows that the device gets through the rejection; the other cases steer draws that every later word depends on."""
    import test_gpu_gkr_rounds as TR
    from tstwo_amd import gkr as G
    from tstwo_amd.gkr_verifier import Gate, partially_verify_batch
    case, state = D.BY_NAME[name], FIX[name]["state"]
    model, (mproof, martifact) = D.run_model(case, state)
    assert steered(model, case)
    layers = D.prove_layers(case.spec)
    n_vars = case.spec or 2
    res = []
    for kw in ({"one_call": True}, {"device_rounds": True}, {"device_rounds": False}):
        dev = [TR.dev_layer(lay) for lay in layers]
        ch = _host_channel(state)
        proof, artifact = G.prove_batch(ch, dev, **kw)
        for d in dev:
            d.free()
        assert TR.to_model(proof, artifact) == (mproof, martifact), kw
        assert [*struct.unpack("<8I", ch.digest()), ch.n_challenges, ch.n_sent] == model.words(), kw
        res.append(proof)
    art = partially_verify_batch([Gate.GrandProduct], res[0], _host_channel(state))
    assert TR.to_model(res[0], art)[1] == martifact
    # the block of the C entry itself: channel, status and the final point
    dev = [TR.dev_layer(lay) for lay in layers]
    inst = (L.GkrInstance * 1)()
    inst[0].kind, inst[0].log_n = M.GP, n_vars
    inst[0].num = (L.vp * 4)(None, None, None, None)
    inst[0].den = (L.vp * 4)(*dev[0].den.ptr_list())
    lay_out = G.one_call_layout([n_vars])
    block = np.zeros(lay_out["words"], dtype=np.uint32)
    L.call("tstwo_gkr_prove_batch", L.u32x(FIX[name]["state"]), inst, 1, block.ctypes.data_as(L.u32p), block.size)
    dev[0].free()
    assert words(block[:10]) == model.words() and int(block[lay_out["status"]]) == 0
    assert [tuple(words(block[lay_out["ood"] + 4 * k:][:4])) for k in range(n_vars)] == martifact["ood_point"]
