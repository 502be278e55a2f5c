"""The schedule of tstwo_gkr_prove_batch restated in Python (csrc/gkr_plan.h says the same in C++; test_cpu_gkr_plan.py compares the
two line by line), the batches the -m gpu file proves, and the plan branches they reach.  It imports nothing from the package.

An instance is (kind, log_n).  Layer L of the proof has L rounds; instance i enters at first = n_layers - log_n and at layer
L >= first its oracle has n_v = L - first variables.  The lanes of a layer are its active instances in instance order."""
from __future__ import annotations

GP, GENERIC, MULT, SINGLES = 0, 1, 2, 3
KINDS = (GP, GENERIC, MULT, SINGLES)
MAX_INSTANCES, MAX_LOG = 64, 28
NO_FOLD, IN_PLACE, NEW, NEW_BASE = "S", "I", "N", "B"


class PlanError(Exception):
    pass


def col_words(k):
    return 4 if k < 2 else 1 << k


def layer_off(gen_off, gen_cols, k):
    return gen_off + gen_cols * sum(col_words(j) for j in range(k))


class Plan:
    def __init__(self, batch):
        batch = list(batch)
        n = len(batch)
        if n == 0:
            raise PlanError("no instances")
        if n > MAX_INSTANCES:
            raise PlanError("prove_batch: 1 to 64 instances")
        for kind, log_n in batch:
            if kind not in KINDS:
                raise PlanError("unknown GKR layer kind")
            if log_n == 0:
                raise PlanError("Some output claims were not set during proving (an input layer of 0 variables is an output layer)")
            if log_n > MAX_LOG:
                raise PlanError("GKR layer too large")
            if kind == MULT and log_n == 1:
                raise PlanError("LogUpMultiplicities should never reach tryIntoMask")
        self.batch, self.n = batch, n
        self.n_layers = max(log_n for _, log_n in batch)
        self.first = [self.n_layers - log_n for _, log_n in batch]
        self.gen_cols = [4 if kind == GP else 8 for kind, _ in batch]
        self.gen_off, pool = [], 0
        for (kind, log_n), cols in zip(batch, self.gen_cols):
            self.gen_off.append(pool)
            pool = layer_off(pool, cols, log_n)
        self.pool_words = pool
        self.state_off = 32
        self.sums_off = self.state_off + 8 * n
        self.ctv_off = self.sums_off + 8 * n
        self.out_off = self.ctv_off + 8 * n
        self.ood_off = [self.out_off + 8 * n, self.out_off + 8 * n + 4 * self.n_layers]
        self.inv_off = self.ood_off[1] + 4 * self.n_layers
        self.final_ood = self.ood_off[self.n_layers & 1]
        off = self.inv_off + 4 * self.n_layers
        self.layers = []
        for L in range(self.n_layers):
            active = [i for i in range(n) if self.n_v(i, L) >= 0]
            enter = [i for i in active if self.n_v(i, L) == 0]
            self.layers.append({"n_rounds": L, "active": active, "enter": enter, "poly_off": off, "mask_off": off + 20 * L})
            off += 20 * L + 16 * len(active)
        self.block_words = off

    def n_v(self, i, L):
        return L - self.first[i]

    def fold_kind(self, i, L, f):
        """Fold number f of the layer instance i reduces at layer L: only the last layer reduces the caller's layers, whose first
        fold goes to a new place."""
        if L + 1 != self.n_layers or f:
            return IN_PLACE
        return NEW_BASE if self.batch[i][0] == MULT else NEW

    def round_fold(self, i, L, rem):
        n_v = self.n_v(i, L)
        return NO_FOLD if rem == n_v else self.fold_kind(i, L, n_v - rem - 1)

    def last_fold(self, i, L):
        return self.fold_kind(i, L, self.n_v(i, L) - 1)

    def round_lanes(self, L, rem):
        return [j for j, i in enumerate(self.layers[L]["active"]) if self.n_v(i, L) >= rem]


def _bits(idx):
    return sum(1 << i for i in idx)


def render(p):
    """One line per batch, the format of tests/gkr_plan_main.cpp."""
    out = [f"layers={p.n_layers} block={p.block_words} pool={p.pool_words} off={p.state_off},{p.sums_off},{p.ctv_off},{p.out_off},"
           f"{p.ood_off[0]},{p.ood_off[1]},{p.inv_off},{p.final_ood} gen=" + ",".join(f"{o}/{c}" for o, c in zip(p.gen_off, p.gen_cols))]
    for L, lay in enumerate(p.layers):
        s = f"L{L}:{lay['n_rounds']}:{_bits(lay['enter']):x}:{_bits(lay['active']):x}:{lay['poly_off']}:{lay['mask_off']}"
        for rem in range(L, 0, -1):
            lanes = p.round_lanes(L, rem)
            s += f" r{rem}={_bits(lanes):x}/"
            for j, i in enumerate(lay["active"]):
                s += f"{min(p.n_v(i, L), rem)}{p.round_fold(i, L, rem) if j in lanes else '-'}"
        s += " last=" + "".join(p.last_fold(i, L) if p.n_v(i, L) >= 1 else "-" for i in lay["active"])
        out.append(s)
    return " | ".join(out)


def branches(p):
    """The plan branches a batch reaches."""
    b = set()
    b.add("one instance" if p.n == 1 else "64 instances" if p.n == 64 else "several instances")
    for i, f in enumerate(p.first):
        b.add("enters at the first layer" if f == 0 else "enters at the last layer" if f == p.n_layers - 1 else "enters at a middle layer")
    for L, lay in enumerate(p.layers):
        if lay["n_rounds"] == 0:
            b.add("a layer with zero rounds")
        if lay["enter"] and len(lay["enter"]) < len(lay["active"]):
            b.add("an entering instance beside continuing ones")
        for i in lay["active"]:
            n_v = p.n_v(i, L)
            if L - n_v in (0, 1, 12):                   # the claim is doubled n_rounds - n_v times
                b.add("shift %d" % (L - n_v))
            for f in range(n_v):
                k = p.fold_kind(i, L, f)
                b.add({IN_PLACE: "fold in place", NEW: "fold into a new buffer", NEW_BASE: "base numerators"}[k])
    return b


ALL_BRANCHES = {"one instance", "64 instances", "several instances", "enters at the first layer", "enters at a middle layer",
                "enters at the last layer", "a layer with zero rounds", "an entering instance beside continuing ones", "shift 0", "shift 1",
                "shift 12", "fold in place", "fold into a new buffer", "base numerators"}


# ---------------------------------------------------------------- the batches of the -m gpu files
def named_batch(name):
    """The shapes of test_gpu_gkr_rounds.case_layers."""
    if name == "mixed":
        return [(GENERIC, 13), (GP, 1), (SINGLES, 7), (MULT, 4), (GP, 10)]
    if name == "64":
        return [(KINDS[i % 4], 2 + (i % 3 == 0)) for i in range(64)]
    if name == "65":
        return [(KINDS[i % 4], 3) for i in range(65)]
    if name == "small":
        return [(GENERIC, 4), (GP, 2), (SINGLES, 3)]
    return [name]


def gpu_batches():
    """Every batch tests/test_gpu_gkr_one_call.py proves in one call."""
    out = {str((k, n)): named_batch((k, n)) for k in KINDS for n in (1, 2, 3, 6, 13) if not (k == MULT and n == 1)}
    for name in ("mixed", "64", "small"):
        out[name] = named_batch(name)
    return out
