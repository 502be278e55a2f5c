"""Blake2sChannel.draw_felt at the edges of its rejection rule: the model, the planted faults and the case lists.

A draw hashes digest || LE32(n_sent) || 0^28, advances n_sent, and repeats while any of the 8 words is >= 2P; the felt is the
first four words reduced.  A rejection has probability 2^-28, so the states that meet one (or that put P or 2P - 1 into a word)
are searched for on the CPU (tools/draw_edge_search.c, driven by tools/make_draw_edge_fixtures.py) and committed in
tests/golden/blake2s_draw_edges.json.  tests/test_cpu_draw_edges.py proves the fixtures on raw hash words, holds
tstwo_amd/channel.py to the model and kills every planted fault with every entry's list; tests/test_gpu_draw_edges.py sends
the same cases through every device entry that draws.

The model is written on hashlib alone and imports nothing from the package under test."""
from __future__ import annotations

import collections
import functools
import hashlib
import json
import os
import struct
import zlib

import numpy as np

P = 2**31 - 1
TAG = 0xD4A3ED6E                      # word 0 of every searched digest (tools/draw_edge_search.c)
FIXTURE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blake2s_draw_edges.json")
DEVICE_TRIES = 64                     # the bound of the device loop (csrc/blake2s.cuh); no fixture needs more than two hashes

# ---------------------------------------------------------------- the draw, and its planted faults
FAULTS = {
    "a": "no retry",
    "b": "tests words 0..3 only",
    "c": "bound <= 2P",
    "d": "bound < 2P - 1",
    "e": "n_sent not advanced on a rejection",
    "f": "reduction with > for >=",
    "g": "after a rejection, the felt comes from the rejected words",
}


def hash_words(digest: bytes, n_sent: int):
    return list(struct.unpack("<8I", hashlib.blake2s(digest + struct.pack("<I", n_sent) + bytes(28)).digest()))


def draw(digest: bytes, n_sent: int, fault=None):
    """(felt, n_sent after, hashes taken); fault: a key of FAULTS, each changes one line"""
    first = None
    for hashes in range(1, DEVICE_TRIES + 1):
        w = hash_words(digest, n_sent)
        first = first or w
        tested = w[:4] if fault == "b" else w
        ok = all((x <= 2 * P) if fault == "c" else (x < 2 * P - 1) if fault == "d" else (x < 2 * P) for x in tested)
        if ok or fault != "e":
            n_sent = (n_sent + 1) & 0xFFFFFFFF
        if ok or fault == "a":
            break
    src = first if fault == "g" else w
    felt = tuple(x - P if ((x > P) if fault == "f" else (x >= P)) else x for x in src[:4])
    return felt, n_sent, hashes


class Channel:
    """The transcript on the model's draw: the interface of gkr_model.Channel plus mix_root and the counters."""

    def __init__(self, state=None, fault=None):
        state = [0] * 10 if state is None else state
        self.digest = struct.pack("<8I", *state[:8])
        self.n_challenges, self.n_sent = int(state[8]), int(state[9])
        self.fault = fault
        self.draws = []               # per draw: (digest, n_sent on entry, hashes taken)
        self.mixes = []               # per mix: the bytes hashed behind the digest

    def _mix(self, payload: bytes):
        self.mixes.append(payload)
        self.digest = hashlib.blake2s(self.digest + payload).digest()
        self.n_challenges = (self.n_challenges + 1) & 0xFFFFFFFF
        self.n_sent = 0

    def mix_root(self, root: bytes):
        self._mix(bytes(root))

    def mix_felts(self, felts):
        self._mix(b"".join(struct.pack("<4I", *f) for f in felts))

    def draw_felt(self):
        felt, after, hashes = draw(self.digest, self.n_sent, self.fault)
        self.draws.append((self.digest, self.n_sent, hashes))
        self.n_sent = after
        return felt

    def words(self):
        return list(struct.unpack("<8I", self.digest)) + [self.n_challenges, self.n_sent]


# ---------------------------------------------------------------- conditions on the first hash of the steered draw
# name -> (word range, values, rejected)
CONDITIONS = {
    "rej_lo_2P": (range(0, 4), (2 * P,), True), "rej_lo_max": (range(0, 4), (2 * P + 1,), True),
    "rej_lo": (range(0, 4), (2 * P, 2 * P + 1), True), "rej_hi_2P": (range(4, 8), (2 * P,), True),
    "rej_hi_max": (range(4, 8), (2 * P + 1,), True), "rej_hi": (range(4, 8), (2 * P, 2 * P + 1), True),
    "rej": (range(0, 8), (2 * P, 2 * P + 1), True), "acc_lo_top": (range(0, 4), (2 * P - 1,), False),
    "acc_hi_top": (range(4, 8), (2 * P - 1,), False), "acc_P": (range(0, 4), (P,), False),
}
STANDALONE_CONDS = ["rej_lo_2P", "rej_lo_max", "rej_hi_2P", "rej_hi_max", "acc_lo_top", "acc_hi_top", "acc_P", "rej_lo_2P@s=5"]


def condition_word(cond, w):
    """the index of the first word of the hash w that meets cond (as the search tool reports it), or None"""
    words, values, rejected = CONDITIONS[cond]
    k = next((i for i in words if w[i] in values), None)
    if k is None or rejected == all(x < 2 * P for x in w):
        return None
    if rejected and words[0] == 4 and any(x >= 2 * P for x in w[:4]):
        return None
    return k


# ---------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "name entry cond n_sent target spec")
N_CHALLENGES = 3
ROOT = bytes((7 * 3 + 5 * k) & 0xFF for k in range(32))          # the root the stand-alone entry mixes


def _cases():
    out = []
    for entry in ("draw", "mix"):
        for c in STANDALONE_CONDS:
            cond, _, s = c.partition("@s=")                 # n_sent = 5 on entry: draw only, the counter rides through the rejection;
                                                            # behind a mix, it pins that the mix resets it before the rejected hash
            out.append(Case(f"{entry}/{c}", entry, cond, int(s or 0), 0, None))
    for cond in ("rej_lo", "rej_hi", "acc_lo_top", "acc_P"):
        out.append(Case(f"fri/3/alpha0/{cond}", "fri", cond, 0, 0, (3,)))
    for logs, target in (((3,), 1), ((3,), 2), ((4, 3), 1)):
        for cond in ("rej_lo", "rej_hi"):
            out.append(Case(f"fri/{'.'.join(map(str, logs))}/alpha{target}/{cond}", "fri", cond, 0, target, logs))
    for n in (1, 3):
        for cond in ("rej_lo", "rej_hi", "acc_lo_top"):
            out.append(Case(f"finish/{n}/{cond}", "finish", cond, 0, 0, n))
    out.append(Case("finish/1/acc_P", "finish", "acc_P", 0, 0, 1))
    for lane in ("gp", "logup"):
        for target in (0, 1):
            out.append(Case(f"begin/{lane}/draw{target}", "begin", "rej", 2, target, lane))
    # beyond the issue's table, so that the list kills every fault: a rejection at exactly 2P, and the two accepted edges
    out.append(Case("begin/gp/rej_lo_2P", "begin", "rej_lo_2P", 2, 0, "gp"))
    out.append(Case("begin/logup/acc_lo_top", "begin", "acc_lo_top", 2, 1, "logup"))
    out.append(Case("begin/gp/acc_P", "begin", "acc_P", 2, 1, "gp"))
    for lane in ("gp", "logup"):
        for cond in ("rej_lo", "rej_hi"):
            out.append(Case(f"end/{lane}/{cond}", "end", cond, 1, 0, lane))
    out.append(Case("end/gp/acc_lo_top", "end", "acc_lo_top", 1, 0, "gp"))
    out.append(Case("end/logup/acc_P", "end", "acc_P", 1, 0, "logup"))
    # prove_batch of one grand-product instance of 2^2 inputs draws: 0 alpha, 1 lambda (layer 0's begin), 2 r (its end), 3 alpha,
    # 4 lambda (layer 1's begin), 5 the only sum-check round's challenge, 6 layer 1's end
    out.append(Case("prove/begin0", "prove", "rej", 0, 0, None))
    out.append(Case("prove/round0", "prove", "rej", 0, 5, None))
    for cond in ("rej_lo_2P", "acc_lo_top"):                          # the first layer_end's draw: every later word depends on it
        out.append(Case(f"prove/end0/{cond}", "prove", cond, 0, 2, None))
    # a drawn P is 0 to all arithmetic that follows; it shows only where the proof hands a draw out as drawn, in the final
    # out-of-domain point.  An instance of 2^1 inputs has one layer: its layer_end draw (2) is that point.
    out.append(Case("prove/1var/acc_P", "prove", "acc_P", 0, 2, 1))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# The lists the device entries are run on (tests/test_gpu_draw_edges.py); each kills every planted fault on its own
# (test_cpu_draw_edges.py).
ENTRY_LISTS = {
    "channel draw": [c.name for c in CASES if c.entry == "draw"],
    "channel mix+draw": [c.name for c in CASES if c.entry == "mix"],
    "fri commit": [c.name for c in CASES if c.entry == "fri"],
    "gkr round_finish": [c.name for c in CASES if c.entry == "finish"],
    "gkr layer_begin": [c.name for c in CASES if c.entry == "begin"],
    "gkr layer_end": [c.name for c in CASES if c.entry == "end"],
    "gkr prove_batch": [c.name for c in CASES if c.entry == "prove"],
}
# Cases whose steered draw no output of the entry depends on, so that no fault of the draw can show in them
# (test_cpu_draw_edges.py proves it on the model: NO fault changes their outcome).  The alpha and lambda that prove_batch's first
# layer_begin draws feed only the sum-check rounds of that layer, and layer 0 has none, for any batch (layer L runs L rounds); the
# mask mix that follows resets n_sent and hashes the digest, which no draw changes.  The case stays because the issue names it:
# it shows that the device gets through a rejected draw there and leaves the rest of the proof as it is.
UNOBSERVABLE = {"prove/begin0": "layer 0 has no sum-check round: its alpha and lambda feed nothing"}


def salt(case):
    return zlib.crc32(case.name.encode())


def load_fixtures():
    with open(FIXTURE_PATH) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------- the inputs of every entry, from seeds
@functools.lru_cache(maxsize=None)
def _fri_columns(col_logs):
    from oracle import oracle as orc
    cols = []
    for j, c in enumerate(col_logs):
        half = orc.lib().orc_half_odds_initial(c - 1)
        tw = orc.precompute_twiddles(half, c - 1)[0]
        coords = []
        for i in range(4):
            coeffs = np.zeros(1 << c, dtype=np.uint32)
            coeffs[:1 << (c - 1)] = np.random.default_rng(8100 + 40 * j + 4 * c + i).integers(0, P, size=1 << (c - 1), dtype=np.uint32)
            coords.append(orc.cfft_evaluate(coeffs, c, half, tw, c - 1))
        cols.append(coords)
    return cols


def fri_columns(col_logs):
    """per circle column its four coordinate columns: evaluations on the canonic domain of log c of polynomials of half its size
    (blowup 2), so that FriProver.commit and FriVerifier take them too"""
    return [[c.copy() for c in col] for col in _fri_columns(tuple(col_logs))]


def _felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def finish_inputs(n):
    """claims, corrections and one round (as test_gpu_gkr_rounds.random_round) of n instances; the middle one of three is inactive"""
    rng = np.random.default_rng(9100 + n)
    rd = {"sums": [(_felt(rng), _felt(rng)) for _ in range(n)], "active": [i != 1 for i in range(n)], "y": _felt(rng), "a": _felt(rng),
          "alpha": _felt(rng)}
    return [_felt(rng) for _ in range(n)], [_felt(rng) for _ in range(n)], rd


GP, GENERIC = 0, 1                    # gkr_model.GP / GENERIC (asserted in test_cpu_draw_edges.py)


def lane_inputs(lane):
    """One lane, as test_gpu_gkr_one_call.Lanes lays it out: instance 1 of 4; 16 columns of 3 words (8 src, 8 out_src).  The
    grand-product lane continues (its claim comes from `claims`), the LogUp lane enters (its claims are its output values)."""
    rng = np.random.default_rng(9200 + (lane == "logup"))
    kind = GP if lane == "gp" else GENERIC
    cols = rng.integers(0, P, size=(1, 16, 3), dtype=np.uint64)
    y = [_felt(rng) for _ in range(2)]
    claims = {} if lane == "logup" else {1: [_felt(rng)]}
    return {"kind": kind, "enter": lane == "logup", "inst": 1, "shift": 1, "cols": cols, "y": y, "claims": claims,
            "lanes": [{"inst": 1, "kind": kind, "shift": 1, "enter": lane == "logup"}]}


def lane_value(cols, first_col, word):
    return tuple(int(cols[0, first_col + c, word]) for c in range(4))


def prove_layers(n_vars=None):
    """one grand-product instance of 2^2 inputs (or of 2^n_vars), as a gkr_model layer"""
    n_vars = n_vars or 2
    rng = np.random.default_rng(9300 + (n_vars != 2) * n_vars)
    return [{"kind": GP, "num": None, "den": rng.integers(0, P, size=(4, 1 << n_vars), dtype=np.uint64)}]


# ---------------------------------------------------------------- every entry on the model channel
def fri_commit_model(col_logs, state, fault=None, last=0):
    """FriProver.commit's layer loop on the CPU oracle and the model channel (as test_gpu_bounds.test_fri_commit_layers replays it):
    (channel, first tree, [(log, evaluation, tree or None)], alphas)"""
    from oracle import oracle as orc
    half_odds = orc.lib().orc_half_odds_initial
    cols = fri_columns(col_logs)
    ch = Channel(state, fault)
    log = col_logs[0]
    tw_log = log + 1
    half_initial = lambda c: (half_odds(tw_log) << (tw_log - c + 1)) & 0x7FFFFFFF      # noqa: E731
    first_layers, root = orc.merkle_commit([c for col in cols for c in col], [c for c in col_logs for _ in range(4)])
    ch.mix_root(root)
    alphas = [ch.draw_felt()]
    cur = orc.fold_circle_into_line(orc.soa_alloc(1 << (log - 1)), cols[0], log, half_initial(log), alphas[-1])
    joining = {c - 1: col for c, col in zip(col_logs[1:], cols[1:])}
    layers = []
    for lg in range(log - 1, last, -1):
        tree, root = orc.merkle_commit(cur, [lg] * 4)
        layers.append((lg, cur, np.concatenate(tree)))
        ch.mix_root(root)
        alphas.append(ch.draw_felt())
        cur = orc.fold_line(cur, lg, (half_odds(tw_log) << (tw_log - lg)) & 0x7FFFFFFF, alphas[-1])
        if lg - 1 in joining:
            cur = orc.fold_circle_into_line(cur, joining.pop(lg - 1), lg, half_initial(lg), alphas[-1])
    assert not joining
    layers.append((last, cur, None))
    return ch, np.concatenate(first_layers), layers, alphas


def run_model(case, state, fault=None):
    """(channel after the entry, everything else the entry puts out) on the model"""
    import gkr_layer_model as LM
    import gkr_model as M
    import gkr_round_model as R
    ch = Channel(state, fault)
    if case.entry == "draw":
        return ch, ch.draw_felt()
    if case.entry == "mix":
        ch.mix_root(ROOT)
        return ch, ch.draw_felt()
    if case.entry == "fri":
        ch, first, layers, alphas = fri_commit_model(list(case.spec), state, fault)
        return ch, (first.tobytes(), [(lg, [c.tolist() for c in ev], None if t is None else t.tobytes()) for lg, ev, t in layers], alphas)
    if case.entry == "finish":
        claims, corrs, rd = finish_inputs(case.spec)
        return ch, R.round_finish_at(ch, rd["sums"], claims, corrs, rd["active"], rd["y"], rd["a"], rd["alpha"])
    if case.entry in ("begin", "end"):
        ln = lane_inputs(case.spec)
        claims = [None] * 4
        for i, c in ln["claims"].items():
            claims[i] = list(c)
        if case.entry == "begin":
            den = lane_value(ln["cols"], 12, 0)
            outputs = {1: [den] if ln["kind"] == GP else [lane_value(ln["cols"], 8, 0), den]}
            return ch, (LM.layer_begin(ch, ln["lanes"], claims, outputs, ln["y"]), claims)
        mask = LM.mask_of(ln["kind"], (lane_value(ln["cols"], 0, 0), lane_value(ln["cols"], 0, 1)),
                          (lane_value(ln["cols"], 4, 0), lane_value(ln["cols"], 4, 1)))
        return ch, (LM.layer_end(ch, ln["lanes"], [mask], claims), mask, claims)
    assert case.entry == "prove"
    return ch, M.prove_batch(ch, prove_layers(case.spec))


def search_arguments(case, workdir):
    """the search tool's arguments that describe the transcript before the steered draw (no salt, walk or bound)"""
    args = ["--cond", case.cond, "--n-sent", str(case.n_sent)]
    if case.entry == "fri":
        path = os.path.join(workdir, "cols_" + "_".join(map(str, case.spec)) + ".bin")
        with open(path, "wb") as f:
            for col in fri_columns(case.spec):
                for c in col:
                    f.write(c.astype("<u4").tobytes())
        return args + ["--fri", ",".join(map(str, case.spec)), "--cols", path, "--draw", str(case.target)]
    if case.entry == "prove" and case.target == 5:
        den = prove_layers()[0]["den"]
        return args + ["--gkr-gp", b"".join(struct.pack("<4I", *(int(v) for v in den[:, i])) for i in range(4)).hex()]
    # every other entry mixes inputs that do not depend on the channel: take them from a model run on any state
    ch, _ = run_model(case, [0] * 10)
    # prove_batch: the mixes before draw 0 (the output) or draw 2 (the output, the mask; the two draws between them change neither
    # the digest nor, behind the second mix, n_sent)
    n_mixes = len(ch.mixes) if case.entry != "prove" else 1 + (case.target == 2)
    for payload in ch.mixes[:n_mixes]:
        args += ["--mix", payload.hex()]
    return args + ["--pre-draws", str(0 if case.entry == "prove" else case.target)]
