"""The tests' own statement of the Circle FFT's launch plan (no GPU, no library): which kernels an entry launches for n_cols columns of
2^n words on a device of n_cus compute units, on which tiles, with how many lanes and how much LDS.

Written from the code as it stood before csrc/cfft_plan.h existed, where five places each decided a part: the cut of the layers
(plan_passes), the default shape per size (default_shape), the few-column choice and the experiments build's knobs (choose_plan), the
kernel per pass (the switches of launch_fast, which also chose the non-temporal kernels) and the out-of-place entries' own bodies.
This module keeps that order — shape, cut, then one kernel per pass in launch order, refusing at the first pass without one —
while the header states the plan as one function over a table.  tests/test_cpu_cfft_plan.py compares the two.

Differences from that code, all on purpose: a plan is refused as a whole before anything is launched; a plan of more than 8 passes
(TSTWO_CFFT_KA = 1 or 2 on large sizes overran the pass array) is refused; k_cfft_a<., 1, 0, 12> and the fused extension with 10
layers on the 2^14 tile, which no input or single knob reached, have no kernel any more; the routes below n = 13 refuse a column
count past 32 bits, which their kernels truncated ("cfft: grid too large" came later than that and is gone)."""
from collections import namedtuple

MAX_LOG, MAX_PASSES = 30, 8
ENTRIES = ("evaluate", "interpolate", "interpolate_to", "evaluate_extended")
KINDS = ("whole", "bottom", "bottom_stream", "bottom_oop", "strided", "strided_stream", "strided_ext")
ROUTES = ("small", "generic", "tiled", "fallback")
NO_KNOBS = (0, 0, 0)

Pass = namedtuple("Pass", "kind lo k logt threads lds tiles scale")
Plan = namedtuple("Plan", "route cols_per_wg blocks passes")

# (kind, K, LOGT) with a kernel -> whether only TSTWO_CFFT_KB / KA / LOGTA of the experiments build reach it
TABLE = {("bottom", 11, 11): True, ("bottom", 12, 12): False, ("bottom", 13, 13): False, ("bottom", 14, 14): False,
         ("bottom_stream", 13, 13): False, ("bottom_stream", 14, 14): False, ("bottom_oop", 13, 13): False, ("bottom_oop", 14, 14): False,
         ("strided", 9, 13): False, ("strided", 1, 14): True, ("strided", 10, 14): True}
TABLE.update({("strided", k, 12): False for k in range(2, 9)})
TABLE.update({("strided", k, 14): False for k in range(2, 10)})
TABLE.update({("strided_ext", k, 14): False for k in range(2, 10)})
TABLE.update({(kind, k, 15): False for kind in ("strided", "strided_stream", "strided_ext") for k in (8, 9, 10)})


class PlanError(Exception):
    pass


def streams_past_cache(n_cols, n):
    return (n_cols << n) >= 1 << 28


def default_shape(n, n_cols, n_cus):
    """(bottom tile, layers per strided pass at most, strided tile) of a many-column transform"""
    wide = n >= 15 and (n_cols << (n - 15)) >= 2 * n_cus
    if n == 24:
        return 14, 10, 15
    if n == 23:
        return (13, 10, 15) if wide else (14, 9, 14)
    if n in (21, 22) and wide:
        return 13, 9, 15
    if n == 14:
        return 14, 9, 14
    return 13, 9, 14


def choose_shape(n, n_cols, n_cus, knobs):
    """an in-place transform's: the knobs of the experiments build, else the split with the most workgroups for few columns"""
    kb, ka_max, logta = default_shape(n, n_cols, n_cus)
    knob_kb, knob_ka, knob_logta = knobs
    kb, ka_max = knob_kb or kb, knob_ka or ka_max
    want = 2 * n_cus
    if n > kb and n >= 14 and not knob_kb and not knob_ka and (n_cols << (n - 14)) < want and n - 13 <= ka_max:
        best = 0
        for tb in (13, 12, 11):
            k = n - tb
            ta = 12 if k <= 8 else 13 if k == 9 else 14
            if not 1 <= k <= ka_max or ta > n:
                continue
            score = min(n_cols << (n - ta), n_cols << (n - tb), want)
            if score > best:
                best, kb, logta = score, tb, ta
    return kb, ka_max, knob_logta or logta


def cut(n, kb, ka_max, logta):
    """[(lo, k, logt)] low -> high: the bottom pass, then equal strided passes"""
    if n <= kb:
        return [(0, n, n)]
    out, rem, lo = [(0, kb, kb)], n - kb, kb
    count = -(-rem // ka_max)
    for s in range(count):
        k = rem // count + (1 if s < rem % count else 0)
        out.append((lo, k, min(logta - k, lo) + k))
        lo += k
    return out


def plan(entry, n, n_cols, n_cus=256, knobs=NO_KNOBS, ext=0):
    """The Plan, or PlanError(reason)."""
    if n == 0 or n > 31:
        raise PlanError("cfft: log_size out of range")
    if n > MAX_LOG:
        raise PlanError("cfft: log_size > 30 exceeds MAX_CIRCLE_DOMAIN_LOG_SIZE (poly/circle/domain.ts:4)")
    inverse = entry in ("interpolate", "interpolate_to")
    in_place = entry in ("evaluate", "interpolate")
    fallback = Plan("fallback", 0, 0, [])
    if not in_place and not (n >= 13 and not knobs[0] and not knobs[1]):
        return fallback
    if n <= 2:
        if n_cols > 0xffffffff:
            raise PlanError("cfft: too many (tile, column) work items")
        return Plan("small", 0, (n_cols + 63) // 64, [Pass("whole", 0, n, n, 64, 0, 1, inverse)])
    if n <= 12:
        cpw = 4
        while cpw > 1 and -(-n_cols // cpw) < n_cus * 6:
            cpw //= 2
        cpw = min(cpw, n_cols) or cpw
        if n_cols > 0xffffffff:
            raise PlanError("cfft: too many (tile, column) work items")
        tile, heap = 1 << n, 1 << (n - 1)
        lds = (((tile + tile // 32 + 3) & ~3) + heap + 4) * 4
        return Plan("generic", cpw, -(-n_cols // cpw), [Pass("whole", 0, n, n, 256, lds, 1, inverse)])
    shape = choose_shape(n, n_cols, n_cus, knobs) if in_place else default_shape(n, n_cols, n_cus)
    layers = cut(n, *shape)
    if len(layers) > MAX_PASSES:
        raise PlanError("cfft: more passes than a plan holds")
    if entry == "evaluate_extended" and not (len(layers) >= 2 and ext in (1, 2) and layers[-1][1] >= 2):
        return fallback
    order = layers if inverse else layers[::-1]
    stream = not inverse and streams_past_cache(n_cols, n)
    passes = []
    for i, (lo, k, logt) in enumerate(order):
        first_of_two_tables = i == 0 and not in_place
        if lo == 0:
            kind = "bottom_oop" if first_of_two_tables else "bottom_stream" if stream and k in (13, 14) else "bottom"
            threads, lds = 1 << (k - 4), ((1 << k) + (1 << (k - 5)) + (1 << (k - 4))) * 4
            if (kind, k, logt) not in TABLE:
                raise PlanError("cfft: unsupported bottom pass")
        else:
            kind = "strided_ext" if first_of_two_tables else "strided_stream" if stream and logt == 15 else "strided"
            threads, lds = (1 << (logt - 4)) // (2 if logt == 15 else 1), ((1 << logt) + (1 << (logt - 5)) + (1 << k)) * 4
            if (kind, k, logt) not in TABLE:
                raise PlanError("cfft: unsupported pass shape")
        tiles = 1 << (n - logt)
        if tiles * n_cols > 0xffffffff:
            raise PlanError("cfft: too many (tile, column) work items")
        passes.append(Pass(kind, lo, k, logt, threads, lds, tiles, inverse and i == len(order) - 1))
    return Plan("tiled", 0, 0, passes)


def render(p):
    """One line per plan, as tests/cfft_plan_main.cpp prints the library's."""
    words = [f"{p.route}:{p.cols_per_wg}:{p.blocks}"]
    words += [f"{s.kind}:{s.lo}:{s.k}:{s.logt}:{s.threads}:{s.lds}:{s.tiles}:{int(s.scale)}" for s in p.passes]
    return " ".join(words)


def shapes(p):
    """the (kind, K, LOGT) of a plan's tiled passes"""
    return {(s.kind, s.k, s.logt) for s in p.passes if s.kind != "whole"}


def smallest_case(shape, n_cus, cols, max_bytes):
    """(n, n_cols) of the smallest column set, of at most max_bytes, on which some entry of the shipped build (no knobs) launches
    the (kind, K, LOGT) `shape`; None if there is none."""
    best = None
    for n in range(13, MAX_LOG + 1):
        for n_cols in cols:
            if (4 * n_cols) << n > max_bytes or (best is not None and (n_cols << n, n) >= best[:2]):
                continue
            plans = [plan(e, n, n_cols, n_cus) for e in ENTRIES[:3]] + [plan("evaluate_extended", n, n_cols, n_cus, ext=e) for e in (1, 2)]
            if any(shape in shapes(p) for p in plans):
                best = (n_cols << n, n, n_cols)
    return best and best[1:]
