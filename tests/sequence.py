"""Call sequences: ops, their chained references, a runner and a plug (tests/test_cpu_sequences.py, tests/test_gpu_sequences.py).

The per-call tests run every entry point alone: upload, one call, download.  The library is not stateless between calls
(tstwo_amd/csrc/context.hip: the scratch block, the upload ring, the two pointer-table slots and their host cache, the result
page, the sticky zero flag, the sequence word, the caching allocator, the stream itself), and all of that state is ordered only
by the current stream.  Here a test is a LIST of calls, enqueued back to back with nothing in between that synchronises, and
every buffer is checked once at the end.

  Seq      the buffers (word arrays inside one device allocation) and the ops, in order.
  Op       one library call: the buffers it reads and writes, call(addr) that makes exactly one L.call, and model(state) that
           gives every word it writes from oracle/oracle.py or the integer models (gkr_model, air_model, air_program_model,
           logup_model, poseidon_model).  Ops chain: a buffer written by one op may be read by a later one, and
           Seq.expected() then runs the models in order over the same state, so a reference is chained as the device data is.
  run()    upload the image, synchronise once, [plug], enqueue every op, download once, compare() bit for bit.  A failure
           names the op's index, its entry point, the buffer and the first and last differing word.
  Plug     enqueued work that keeps the stream busy while the host runs ahead: in-place tstwo_cfft_evaluate /
           tstwo_cfft_interpolate pairs over 64 columns of 2^20 words (256 MiB), which leave the data as it was.  The project's
           recorded time for tstwo_cfft_evaluate on 256 x 2^20 is 975 us (profiles/r04_cfft_sweep.txt), a quarter of the columns
           about 0.25 ms, so PLUG_PAIRS = 80 pairs are about 40 ms of device time.  Plug.check() is the precondition of every
           test that relies on it: the host interval from the first enqueue to the return of the last one must be shorter than
           the plug's device time (tstwo_event pair), else the test FAILS -- it does not pass because the plug drained early.

The catalogue: every entry point that ONLY ENQUEUES, established by reading its source (no read-back, no stream or event
synchronisation on any path the shapes here take):
  field_ops.hip  tstwo_m31_add / _sub / _mul / _neg, tstwo_qm31_mul, tstwo_secure_accumulate, tstwo_bit_reverse: argument
                 checks and one launch.  tstwo_{m31,cm31,qm31}_batch_inverse_async: the launch only; the flag is read by
                 tstwo_check_zero_flag alone.
  cfft.hip       tstwo_cfft_evaluate, _interpolate, _interpolate_to, _evaluate_extended, tstwo_poly_extend: launches; beyond 64
                 columns fill_col_table uploads the pointer table through small_h2d, whose ring path (<= 16 KiB) copies into a
                 page-locked slot and enqueues -- it waits for a slot's event only when the ring wraps onto a copy still pending.
  fri.hip        tstwo_fri_fold_line_dev / _tw / _rows, tstwo_fri_fold_circle_into_line_dev / _tw / _rows: argument checks and one
                 launch (fold_line / fold_circle, the one path of all eight fold entries), alpha by value or read on the device.
  merkle.hip     tstwo_merkle_commit and tstwo_merkle_commit_many with root(s) NULL ("then nothing is synchronised"),
                 tstwo_merkle_commit_layer; poseidon.hip tstwo_poseidon252_merkle_commit with root NULL.  Up to 64 columns the
                 tables travel by value.
  quotients.hip  tstwo_quotients_accumulate_async, tstwo_quotients_accumulate_samples_async: constants blob into the scratch
                 through small_h2d (the blobs here are far below 16 KiB), launches, no flag read.
  gkr_ops.hip    tstwo_gkr_next_layer_*, tstwo_mle_fix_first_variable_*: one launch.  tstwo_gkr_sum_poly_async, tstwo_gkr_round:
                 hipMemsetAsync of the ticket in the scratch, one launch.  tstwo_gkr_gen_eq_evals: two launches via the scratch.
  air.hip        tstwo_air_wide_fib_trace, tstwo_air_constraint_quotients (coefficients by value), tstwo_air_eval_program
                 (program through small_h2d into the scratch).   logup.hip  tstwo_logup_column (descriptors likewise).
  context.hip    tstwo_copy, tstwo_zero (hipMemcpyAsync / hipMemsetAsync), tstwo_upload of at most 16 KiB (the ring).
Left out because they read back or synchronise: every call with a host result (roots, lambda, eval_at_point, gathers,
decommits, grinding, the synchronous inverses and quotients, tstwo_logup_finalize_last, tstwo_download*), tstwo_upload above
16 KiB, tstwo_twiddles_build with itw (a synchronous inverse).

Ops with `capturable` set upload no host array, so they may be recorded into a graph: at most 64 columns, no quotient, AIR
program or LogUp call, no tstwo_upload.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import time

import numpy as np

from oracle import oracle as orc
import air_model as AM
import air_program_model as XM
import gkr_model as GM
import logup_model as LM
import poseidon_model as PM

P = 2147483647
SENTINEL = 0xA5A5A5A5          # above P; every word no upload covers, outputs included
ALIGN = 256                    # bytes; every buffer starts on this boundary of the arena
PLUG_PAIRS = 80
PLUG_LOG = 20
PLUG_COLS = 64
ALPHA = (19283, 1, 2, 3)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_golden.json")


def OL():
    return orc.lib()


def half_odds(k):
    return OL().orc_half_odds_initial(k)


@functools.lru_cache(maxsize=None)
def otwiddles(log):
    tw, itw = orc.precompute_twiddles(half_odds(log), log)
    tw.setflags(write=False); itw.setflags(write=False)
    return tw, itw


def u32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.uint32)).reshape(-1)


def coords(a):
    """The coordinate columns of a model array: (4, n) secure or (n,) base."""
    a = np.asarray(a)
    return [u32(a)] if a.ndim == 1 else [u32(a[k]) for k in range(a.shape[0])]


class Op:
    def __init__(self, entry, reads, writes, call, model, capturable=True, scratch=None):
        self.entry, self.reads, self.writes, self.call, self.model = entry, list(reads), list(writes), call, model
        self.capturable, self.scratch = capturable, scratch

    def enqueue(self, addr):
        """Exactly one library call; addr(name) is the buffer's device address."""
        self.call(addr)

    def expected(self, state):
        """{name: words} for every buffer this op writes, from the references, given the state in front of it."""
        out = self.model(state)
        assert sorted(out) == sorted(self.writes), (self.entry, sorted(out), sorted(self.writes))
        return {k: u32(v) for k, v in out.items()}


class Seq:
    """Buffers and ops.  A buffer is `n` words; `data` is what the image holds before the first op (None: sentinel)."""

    def __init__(self):
        self.sizes, self.data, self.ops, self.kind = {}, {}, [], {}
        self._const = {}

    def buf(self, n_words, data=None, kind=None):
        name = f"b{len(self.sizes)}"
        self.sizes[name] = int(n_words)
        if data is not None:
            data = u32(data).copy()
            assert data.size == n_words
            data.setflags(write=False)
        self.data[name] = data
        self.kind[name] = kind
        return name

    def bufs(self, k, n_words):
        return [self.buf(n_words) for _ in range(k)]

    def inputs(self, arrays):
        return [self.buf(u32(a).size, a) for a in arrays]

    def const(self, key, array):
        """One shared input per key (twiddle tables)."""
        if key not in self._const:
            self._const[key] = self.buf(u32(array).size, array)
        return self._const[key]

    def add(self, op):
        for n in op.reads + op.writes:
            assert n in self.sizes, n
        self.ops.append(op)
        return op

    # ---- layout and images
    def layout(self):
        start, cur = {}, 0
        for name, n in self.sizes.items():
            start[name] = cur
            cur += (4 * n + ALIGN - 1) // ALIGN * ALIGN
        return start, max(cur, ALIGN)

    def image(self):
        start, total = self.layout()
        img = np.full(total // 4, SENTINEL, dtype=np.uint32)
        for name, d in self.data.items():
            if d is not None:
                img[start[name] // 4:start[name] // 4 + d.size] = d
        return img

    def initial_state(self):
        return {n: (self.data[n].copy() if self.data[n] is not None else np.full(self.sizes[n], SENTINEL, dtype=np.uint32))
                for n in self.sizes}

    def expected(self):
        """(state, writer): every buffer's words after the whole sequence, and the index of the op that wrote it last."""
        state, writer = self.initial_state(), {}
        for i, op in enumerate(self.ops):
            for name, words in op.expected(state).items():
                assert words.size == self.sizes[name], (i, op.entry, name, words.size, self.sizes[name])
                state[name] = words
                writer[name] = i
        return state, writer

    def split(self, image):
        start, _ = self.layout()
        return {n: image[start[n] // 4:start[n] // 4 + self.sizes[n]] for n in self.sizes}

    def signature(self):
        return [(op.entry, tuple(op.reads), tuple(op.writes)) for op in self.ops]


def compare(seq, got_image, want=None):
    """Differences between a downloaded image and the chained references, as text, in op order: the op's index in the
    sequence, its entry point, the buffer, and the first and last differing word."""
    state, writer = want if want is not None else seq.expected()
    got = seq.split(np.asarray(got_image, dtype=np.uint32))
    msgs = []
    for name in seq.sizes:
        diff = np.flatnonzero(got[name] != state[name])
        if diff.size == 0:
            continue
        a, b = int(diff[0]), int(diff[-1])
        where = f"first differing word {a} (got {int(got[name][a]):#x}, want {int(state[name][a]):#x}), last differing word {b}, " \
                f"{diff.size} of {seq.sizes[name]} words differ"
        if name in writer:
            i = writer[name]
            msgs.append((i, f"op #{i} {seq.ops[i].entry}: output '{name}': {where}"))
        else:
            msgs.append((len(seq.ops), f"buffer '{name}' that no op writes was modified: {where}"))
    return [m for _, m in sorted(msgs)]


# ------------------------------------------------------------------ the device half
def _L():
    from tstwo_amd import _lib as L
    return L


class Plug:
    """PLUG_PAIRS in-place evaluate / interpolate pairs over PLUG_COLS columns of 2^PLUG_LOG words."""

    def __init__(self, pairs=PLUG_PAIRS):
        L = _L()
        self.pairs = pairs
        n = 1 << PLUG_LOG
        self.buf = L.DeviceBuffer(4 * n * PLUG_COLS)
        self.buf.zero()                                   # the zero polynomial stays the zero polynomial: any words would do
        self.tw, self.itw = L.DeviceBuffer(2 * n), L.DeviceBuffer(2 * n)
        tw, itw = otwiddles(PLUG_LOG - 1)
        self.tw.upload(tw); self.itw.upload(itw)
        self.cols = L.ptr_array([self.buf.ptr + 4 * n * i for i in range(PLUG_COLS)])
        self.e0, self.e1 = L.Event(), L.Event()
        L.sync()
        self.t0 = self.t1 = None

    def enqueue(self):
        L = _L()
        half = half_odds(PLUG_LOG - 1)
        self.t0 = time.perf_counter()
        self.e0.record()
        for _ in range(self.pairs):
            L.call("tstwo_cfft_evaluate", self.cols, PLUG_COLS, PLUG_LOG, half, L.vp(self.tw.ptr), PLUG_LOG - 1)
            L.call("tstwo_cfft_interpolate", self.cols, PLUG_COLS, PLUG_LOG, half, L.vp(self.itw.ptr), PLUG_LOG - 1)
        self.e1.record()

    def host_done(self):
        """Call on return of the last enqueue that must run ahead of the plug."""
        self.t1 = time.perf_counter()

    def check(self):
        """The precondition: the host finished enqueueing while the plug was still running.  Returns device ms / host ms."""
        assert self.t0 is not None and self.t1 is not None
        device_ms = self.e0.elapsed_ms(self.e1)
        host_ms = 1e3 * (self.t1 - self.t0)
        self.device_ms, self.host_ms = device_ms, host_ms
        assert host_ms < device_ms, f"the plug drained early: host enqueue interval {host_ms:.2f} ms, plug device time {device_ms:.2f} ms"
        return device_ms / host_ms

    def free(self):
        for b in (self.buf, self.tw, self.itw):
            b.free()


class Arena:
    """One device allocation holding a sequence's image."""

    def __init__(self, seq, image=None):
        L = _L()
        self.seq = seq
        self.start, self.total = seq.layout()
        self.buf = L.DeviceBuffer(self.total)
        assert self.buf.ptr % ALIGN == 0
        self.buf.upload(seq.image() if image is None else image)

    def addr(self, name, byte_offset=0):
        return self.buf.ptr + self.start[name] + byte_offset

    def download(self):
        return self.buf.download(np.uint32, self.total // 4)

    def free(self):
        self.buf.free()


def enqueue_all(seq, addr, ops=None):
    for op in (seq.ops if ops is None else ops):
        op.enqueue(addr)


def run(seq, plug=None):
    """Upload, synchronise once, [plug], enqueue everything, download once, compare.  Returns (image, plug ratio or None)."""
    L = _L()
    want = seq.expected()
    arena = Arena(seq)
    try:
        L.sync()
        if plug is not None:
            plug.enqueue()
        enqueue_all(seq, arena.addr)
        if plug is not None:
            plug.host_done()
        got = arena.download()
        ratio = plug.check() if plug is not None else None
        if plug is not None:
            print(f"plug: device {plug.device_ms:.1f} ms, host {plug.host_ms:.2f} ms")
    finally:
        arena.free()
    msgs = compare(seq, got, want)
    assert not msgs, f"{len(msgs)} buffers differ; " + "; ".join(msgs[:6])
    return got, ratio


# ------------------------------------------------------------------ the catalogue
def _p4(addr, names):
    return _L().p4([addr(n) for n in names])


def _ptrs(addr, names):
    return _L().ptr_array([addr(n) for n in names])


def _call(*a):
    _L().call(*a)


def m31_op(s, op, a, b=None):
    out = s.buf(s.sizes[a], kind="m31")
    n = s.sizes[a]
    if op == "neg":
        s.add(Op("tstwo_m31_neg", [a], [out], lambda A: _call("tstwo_m31_neg", C.c_void_p(A(a)), C.c_void_p(A(out)), n),
                 lambda S: {out: orc.col_op("neg", S[a])}))
    else:
        s.add(Op(f"tstwo_m31_{op}", [a, b], [out],
                 lambda A: _call(f"tstwo_m31_{op}", C.c_void_p(A(a)), C.c_void_p(A(b)), C.c_void_p(A(out)), n),
                 lambda S: {out: orc.col_op(op, S[a], S[b])}))
    return out


def qm31_mul(s, a4, b4):
    n = s.sizes[a4[0]]
    o4 = [s.buf(n, kind="m31") for _ in range(4)]
    s.add(Op("tstwo_qm31_mul", a4 + b4, o4, lambda A: _call("tstwo_qm31_mul", _p4(A, a4), _p4(A, b4), _p4(A, o4), n),
             lambda S: dict(zip(o4, orc.qm31_col_mul([S[x] for x in a4], [S[x] for x in b4])))))
    return o4


def secure_accumulate(s, col4, other4):
    n = s.sizes[col4[0]]
    s.add(Op("tstwo_secure_accumulate", col4 + other4, col4, lambda A: _call("tstwo_secure_accumulate", _p4(A, col4), _p4(A, other4), n),
             lambda S: dict(zip(col4, orc.accumulate([S[x] for x in col4], [S[x] for x in other4])))))
    return col4


def bit_reverse(s, cols):
    n = s.sizes[cols[0]]
    s.add(Op("tstwo_bit_reverse", cols, cols, lambda A: _call("tstwo_bit_reverse", _ptrs(A, cols), len(cols), n),
             lambda S: {c: orc.bit_reverse(S[c]) for c in cols}, capturable=len(cols) <= 64))
    return cols


def _cm31_inverse(a):
    aos = np.ascontiguousarray(np.stack(a, axis=1), dtype=np.uint32)
    out = np.zeros_like(aos)
    rc = OL().orc_cm31_batch_inverse(aos.ctypes.data_as(C.POINTER(orc.CM31)), out.ctypes.data_as(C.POINTER(orc.CM31)), a[0].size)
    assert rc == 0
    return [np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1])]


def batch_inverse_async(s, ins):
    """1, 2 or 4 coordinate columns: m31, cm31, qm31.  The inputs must hold no zero element."""
    L = _L()
    k, n = len(ins), s.sizes[ins[0]]
    outs = [s.buf(n, kind="m31") for _ in range(k)]
    if k == 1:
        s.add(Op("tstwo_m31_batch_inverse_async", ins, outs,
                 lambda A: _call("tstwo_m31_batch_inverse_async", C.c_void_p(A(ins[0])), C.c_void_p(A(outs[0])), n),
                 lambda S: {outs[0]: orc.m31_batch_inverse(S[ins[0]])}))
    elif k == 2:
        s.add(Op("tstwo_cm31_batch_inverse_async", ins, outs,
                 lambda A: _call("tstwo_cm31_batch_inverse_async", L.P2(*[A(x) for x in ins]), L.P2(*[A(x) for x in outs]), n),
                 lambda S: dict(zip(outs, _cm31_inverse([S[x] for x in ins])))))
    else:
        s.add(Op("tstwo_qm31_batch_inverse_async", ins, outs,
                 lambda A: _call("tstwo_qm31_batch_inverse_async", _p4(A, ins), _p4(A, outs), n),
                 lambda S: dict(zip(outs, orc.qm31_batch_inverse([S[x] for x in ins])))))
    return outs


def _cfft_domain(log):
    tw_log = max(log - 1, 1)
    return tw_log, half_odds(log - 1)


def cfft(s, entry, cols, log):
    """In place: entry = "evaluate" | "interpolate"."""
    tw_log, half = _cfft_domain(log)
    inv = entry == "interpolate"
    tw = s.const(("tw", tw_log, inv), otwiddles(tw_log)[1 if inv else 0])
    f = orc.cfft_interpolate if inv else orc.cfft_evaluate
    s.add(Op(f"tstwo_cfft_{entry}", cols + [tw], cols,
             lambda A: _call(f"tstwo_cfft_{entry}", _ptrs(A, cols), len(cols), log, half, C.c_void_p(A(tw)), tw_log),
             lambda S: {c: f(S[c], log, half, S[tw], tw_log) for c in cols}, capturable=len(cols) <= 64))
    return cols


def cfft_interpolate_to(s, src, log, dst=None):
    tw_log, half = _cfft_domain(log)
    tw = s.const(("tw", tw_log, True), otwiddles(tw_log)[1])
    dst = dst or [s.buf(1 << log, kind="m31") for _ in src]
    s.add(Op("tstwo_cfft_interpolate_to", src + [tw], dst,
             lambda A: _call("tstwo_cfft_interpolate_to", _ptrs(A, src), _ptrs(A, dst), len(src), log, half, C.c_void_p(A(tw)), tw_log),
             lambda S: {d: orc.cfft_interpolate(S[c], log, half, S[tw], tw_log) for c, d in zip(src, dst)}, capturable=len(src) <= 64))
    return dst


def poly_extend(s, src, log_src, log_dst):
    dst = s.buf(1 << log_dst, kind="m31")

    def model(S):
        out = np.zeros(1 << log_dst, dtype=np.uint32)
        out[:1 << log_src] = S[src]
        return {dst: out}
    s.add(Op("tstwo_poly_extend", [src], [dst], lambda A: _call("tstwo_poly_extend", C.c_void_p(A(src)), log_src, C.c_void_p(A(dst)), log_dst), model))
    return dst


def cfft_evaluate_extended(s, polys, log_poly, log):
    tw_log, half = _cfft_domain(log)
    tw = s.const(("tw", tw_log, False), otwiddles(tw_log)[0])
    outs = [s.buf(1 << log, kind="m31") for _ in polys]

    def model(S):
        res = {}
        for p, o in zip(polys, outs):
            ext = np.zeros(1 << log, dtype=np.uint32)
            ext[:1 << log_poly] = S[p]
            res[o] = orc.cfft_evaluate(ext, log, half, S[tw], tw_log)
        return res
    s.add(Op("tstwo_cfft_evaluate_extended", polys + [tw], outs,
             lambda A: _call("tstwo_cfft_evaluate_extended", _ptrs(A, polys), log_poly, _ptrs(A, outs), len(polys), log, half, C.c_void_p(A(tw)), tw_log),
             model, capturable=len(polys) <= 64))
    return outs


def _line_setup(k):
    tw_log = max(k, 1) + 2
    return tw_log, (half_odds(tw_log) << (tw_log - k)) & 0x7FFFFFFF, otwiddles(tw_log)[1]


def fold_line(s, entry, in4, k, alpha=ALPHA, rows=None):
    """entry = "dev" | "tw" | "rows".  rows = (row_offset, n_rows): the other rows of `out` keep their (input) words."""
    L = _L()
    n = 1 << k
    tw_log, coset_initial, itw = _line_setup(k)
    reads = list(in4)
    if entry == "tw":
        tw = s.const(("line_tw", k), itw[(1 << tw_log) - n:(1 << tw_log) - n // 2])
    else:
        tw = s.const(("tw", tw_log, True), itw)
    reads.append(tw)
    if entry == "rows":
        ro, nr = rows
        o4 = s.inputs([np.random.default_rng(7000 + k + j).integers(0, P, size=n // 2, dtype=np.uint32) for j in range(4)])
        reads += o4

        def model(S):
            full = orc.fold_line([S[x] for x in in4], k, coset_initial, alpha)
            res = {}
            for j, o in enumerate(o4):
                e = S[o].copy()
                e[ro:ro + nr] = full[j][ro:ro + nr]
                res[o] = e
            return res
        call = lambda A: _call("tstwo_fri_fold_line_rows", L.p4([A(x, 8 * ro) for x in in4]), k, ro, nr, C.c_void_p(A(tw)), tw_log,
                               L.u32x(alpha), L.p4([A(x, 4 * ro) for x in o4]))
        s.add(Op("tstwo_fri_fold_line_rows", reads, o4, call, model))
        return o4
    o4 = [s.buf(n // 2, kind="m31") for _ in range(4)]
    model = lambda S: dict(zip(o4, orc.fold_line([S[x] for x in in4], k, coset_initial, alpha)))
    if entry == "dev":
        al = s.buf(4, np.array(alpha, dtype=np.uint32))
        reads.append(al)
        call = lambda A: _call("tstwo_fri_fold_line_dev", _p4(A, in4), k, C.c_void_p(A(tw)), tw_log, C.c_void_p(A(al)), _p4(A, o4))
    else:
        call = lambda A: _call("tstwo_fri_fold_line_tw", _p4(A, in4), k, C.c_void_p(A(tw)), L.u32x(alpha), _p4(A, o4))
    s.add(Op(f"tstwo_fri_fold_line_{entry}", reads, o4, call, model))
    return o4


@functools.lru_cache(maxsize=None)
def circle_inv_y(n, half_initial):
    inv = []
    for i in range(1 << (n - 1)):
        p = OL().orc_circle_domain_at(half_initial, n - 1, OL().orc_bit_reverse_index(2 * i, n))
        inv.append(pow(p.y, P - 2, P))
    return np.array(inv, dtype=np.uint32)


def fold_circle_into_line(s, entry, dst4, src4, n, alpha=ALPHA, rows=None):
    """In place on dst4.  "dev" / "rows": the domain whose half coset is root(half_odds(n + 1)) doubled twice; "tw": CanonicCoset(n)."""
    L = _L()
    N = 1 << n
    if entry == "tw":
        half_initial = half_odds(n - 1)
        tw = s.const(("circle_tw", n), circle_inv_y(n, half_initial))
        tw_log = 0
    else:
        tw_log = n + 1
        half_initial = (half_odds(n + 1) << 2) & 0x7FFFFFFF
        tw = s.const(("tw", tw_log, True), otwiddles(tw_log)[1])
    reads = dst4 + src4 + [tw]
    full = lambda S: orc.fold_circle_into_line([S[x] for x in dst4], [S[x] for x in src4], n, half_initial, alpha)
    if entry == "rows":
        ro, nr = rows

        def model(S):
            f, res = full(S), {}
            for j, d in enumerate(dst4):
                e = S[d].copy()
                e[ro:ro + nr] = f[j][ro:ro + nr]
                res[d] = e
            return res
        call = lambda A: _call("tstwo_fri_fold_circle_into_line_rows", L.p4([A(x, 4 * ro) for x in dst4]), L.p4([A(x, 8 * ro) for x in src4]),
                               n, ro, nr, C.c_void_p(A(tw)), tw_log, L.u32x(alpha))
    else:
        model = lambda S: dict(zip(dst4, full(S)))
        if entry == "dev":
            al = s.buf(4, np.array(alpha, dtype=np.uint32))
            reads.append(al)
            call = lambda A: _call("tstwo_fri_fold_circle_into_line_dev", _p4(A, dst4), N // 2, _p4(A, src4), n, C.c_void_p(A(tw)), tw_log, C.c_void_p(A(al)))
        else:
            call = lambda A: _call("tstwo_fri_fold_circle_into_line_tw", _p4(A, dst4), N // 2, _p4(A, src4), n, C.c_void_p(A(tw)), L.u32x(alpha))
    s.add(Op(f"tstwo_fri_fold_circle_into_line_{entry}", reads, dst4, call, model))
    return dst4


def _layers_words(max_log):
    return 8 * ((2 << max_log) - 1)


def _digest_words(layers):
    return np.frombuffer(np.ascontiguousarray(np.concatenate(layers)).tobytes(), dtype="<u4")


def merkle_commit(s, cols, logs):
    L = _L()
    layers = s.buf(_layers_words(max(logs)))
    s.add(Op("tstwo_merkle_commit", cols, [layers],
             lambda A: _call("tstwo_merkle_commit", _ptrs(A, cols), L.u32x(logs), len(cols), C.c_void_p(A(layers)), None),
             lambda S: {layers: _digest_words(orc.merkle_commit([S[c] for c in cols], list(logs))[0])}, capturable=len(cols) <= 64))
    return layers


def merkle_commit_many(s, trees):
    """trees = [(cols, logs)]; roots NULL."""
    L = _L()
    outs = [s.buf(_layers_words(max(logs))) for _, logs in trees]

    def call(A):
        reqs, keep = (L.CommitRequest * len(trees))(), []
        for t, (cols, logs) in enumerate(trees):
            cp, lg = _ptrs(A, cols), L.u32x(logs)
            keep += [cp, lg]
            reqs[t] = L.CommitRequest(cp, lg, len(cols), A(outs[t]))
        _call("tstwo_merkle_commit_many", reqs, len(trees), None)
    s.add(Op("tstwo_merkle_commit_many", [c for cols, _ in trees for c in cols], outs, call,
             lambda S: {o: _digest_words(orc.merkle_commit([S[c] for c in cols], list(logs))[0]) for o, (cols, logs) in zip(outs, trees)}))
    return outs


def merkle_commit_layer(s, log, prev, cols):
    out = s.buf(8 << log)

    def model(S):
        pv = None if prev is None else np.frombuffer(S[prev].tobytes(), dtype=np.uint8).reshape(-1, 32)
        return {out: np.frombuffer(np.ascontiguousarray(orc.commit_on_layer(log, pv, [S[c] for c in cols])).tobytes(), dtype="<u4")}
    s.add(Op("tstwo_merkle_commit_layer", cols + ([prev] if prev else []), [out],
             lambda A: _call("tstwo_merkle_commit_layer", log, C.c_void_p(A(prev)) if prev else C.c_void_p(0), _ptrs(A, cols), len(cols), C.c_void_p(A(out))),
             model, capturable=len(cols) <= 64))
    return out


def poseidon_commit(s, cols, log):
    L = _L()
    layers = s.buf(_layers_words(log))

    def model(S):
        expect = PM.commit([S[c].tolist() for c in cols])
        return {layers: np.array([w for lg in range(log + 1) for x in expect[lg] for w in PM.to_words(x)], dtype=np.uint32)}
    s.add(Op("tstwo_poseidon252_merkle_commit", cols, [layers],
             lambda A: _call("tstwo_poseidon252_merkle_commit", _ptrs(A, cols), L.u32x([log] * len(cols)), len(cols), C.c_void_p(A(layers)), None),
             model))
    return layers


@functools.lru_cache(maxsize=None)
def _sample_points(k):
    with open(GOLDEN) as f:
        px, py = json.load(f)["eval_at_point"][0]["point"]
    pts = [(tuple(px), tuple(py))]
    for _ in range(k - 1):                 # further points on the QM31 circle: repeated doubling
        x, y = pts[-1]
        x2 = OL().orc_qm31_mul(orc.q(x), orc.q(x)).tup()
        xy = OL().orc_qm31_mul(orc.q(x), orc.q(y)).tup()
        pts.append((tuple((2 * a - (1 if i == 0 else 0)) % P for i, a in enumerate(x2)), tuple((2 * a) % P for a in xy)))
    return pts


def _quotient_consts(random_coeff, batches):
    off, cidx, abc, bcoef, prx, pry, pix, piy = [0], [], [], [], [], [], [], []
    for px, py, cv in batches:
        alpha = (1, 0, 0, 0)
        for ci, v in cv:
            alpha = OL().orc_qm31_mul(orc.q(alpha), orc.q(random_coeff)).tup()
            out = (orc.QM31 * 3)()
            OL().orc_line_coeffs(orc.SPoint(orc.q(px), orc.q(py)), orc.q(v), orc.q(alpha), out)
            for t in out:
                abc += list(t.tup())
            cidx.append(ci)
        off.append(len(cidx))
        bcoef += list(alpha)
        prx += px[:2]; pry += py[:2]; pix += px[2:]; piy += py[2:]
    return off, cidx, abc, bcoef, prx, pry, pix, piy


def quotients_async(s, cols, log, n_batches, samples, seed=0):
    """tstwo_quotients_accumulate_async (samples False) or tstwo_quotients_accumulate_samples_async over one column list."""
    L = _L()
    rng = np.random.default_rng(9000 + seed)
    batches = [(bx, by, [(c, tuple(int(v) for v in rng.integers(0, P, size=4))) for c in range(len(cols))])
               for bx, by in _sample_points(n_batches)]
    rc, half = (5, 6, 7, 8), half_odds(log - 1)
    o4 = [s.buf(1 << log, kind="m31") for _ in range(4)]
    if samples:
        entry = "tstwo_quotients_accumulate_samples_async"
        off, cidx, points, values = [0], [], [], []
        for bx, by, cv in batches:
            points += [*bx, *by]
            for ci, v in cv:
                cidx.append(ci)
                values += list(v)
            off.append(len(cidx))
        call = lambda A: _call(entry, half, log, _ptrs(A, cols), len(cols), len(batches), L.u32x(off), L.u32x(cidx), L.u32x(points),
                               L.u32x(values), L.u32x(rc), _p4(A, o4))
    else:
        entry = "tstwo_quotients_accumulate_async"
        off, cidx, abc, bcoef, prx, pry, pix, piy = _quotient_consts(rc, batches)
        call = lambda A: _call(entry, half, log, _ptrs(A, cols), len(cols), len(batches), L.u32x(off), L.u32x(cidx), L.u32x(abc),
                               L.u32x(bcoef), L.u32x(prx), L.u32x(pry), L.u32x(pix), L.u32x(piy), _p4(A, o4))
    s.add(Op(entry, cols, o4, call, lambda S: dict(zip(o4, orc.accumulate_quotients(half, log, [S[c] for c in cols], rc, batches))),
             capturable=False, scratch="quotient blob"))
    return o4


# ---- GKR / MLE: a layer is {"kind", "num": names or None, "den": names}
def _model_layer(S, kind, num, den):
    sec = lambda ns: np.stack([S[x] for x in ns]).astype(np.uint64)
    m = {GM.GENERIC: (lambda: sec(num)), GM.MULT: (lambda: S[num[0]].astype(np.uint64))}.get(kind)
    return {"kind": kind, "num": m() if m else None, "den": sec(den)}


def _num_p4(A, kind, num):
    L = _L()
    if kind == GM.GENERIC:
        return _p4(A, num)
    if kind == GM.MULT:
        return L.p4([A(num[0])] * 4)
    return L.p4([0] * 4)


def gkr_layer_inputs(s, rng, kind, n_vars):
    n = 1 << n_vars
    num = {GM.GENERIC: lambda: s.inputs(coords(GM.random_secure(rng, n))), GM.MULT: lambda: s.inputs(coords(GM.random_base(rng, n)))}.get(kind)
    return (num() if num else None), s.inputs(coords(GM.random_secure(rng, n)))


def gkr_gen_eq_evals(s, y, v):
    L = _L()
    n_y = len(y)
    o4 = [s.buf(1 << n_y, kind="m31") for _ in range(4)]
    s.add(Op("tstwo_gkr_gen_eq_evals", [], o4,
             lambda A: _call("tstwo_gkr_gen_eq_evals", L.u32x([w for t in y for w in t]), n_y, L.u32x(v), _p4(A, o4)),
             lambda S: dict(zip(o4, coords(GM.gen_eq_evals(y, v)))), scratch="gkr eq tables"))
    return o4


def gkr_next_layer(s, kind, num, den, log_n):
    half = 1 << (log_n - 1)
    od = [s.buf(half, kind="m31") for _ in range(4)]
    if kind == GM.GP:
        s.add(Op("tstwo_gkr_next_layer_grand_product", den, od,
                 lambda A: _call("tstwo_gkr_next_layer_grand_product", _p4(A, den), log_n, _p4(A, od)),
                 lambda S: dict(zip(od, coords(GM.next_layer(_model_layer(S, kind, num, den))["den"])))))
        return None, od
    on = [s.buf(half, kind="m31") for _ in range(4)]

    def model(S):
        w = GM.next_layer(_model_layer(S, kind, num, den))
        return dict(zip(on + od, coords(w["num"]) + coords(w["den"])))
    s.add(Op("tstwo_gkr_next_layer_logup", (num or []) + den, on + od,
             lambda A: _call("tstwo_gkr_next_layer_logup", kind, _num_p4(A, kind, num), _p4(A, den), log_n, _p4(A, on), _p4(A, od)), model))
    return on, od


def gkr_sum_poly_async(s, kind, eq4, num, den, n_vars, lam):
    L = _L()
    res = s.buf(8)

    def model(S):
        f0, f2 = GM.sum_f0_f2(_model_layer(S, kind, num, den), np.stack([S[x] for x in eq4]).astype(np.uint64), n_vars, lam)
        return {res: np.array(tuple(f0) + tuple(f2), dtype=np.uint32)}
    s.add(Op("tstwo_gkr_sum_poly_async", eq4 + (num or []) + den, [res],
             lambda A: _call("tstwo_gkr_sum_poly_async", kind, _p4(A, eq4), _num_p4(A, kind, num), _p4(A, den), n_vars, L.u32x(lam), C.c_void_p(A(res))),
             model, scratch="gkr ticket and slab"))
    return res


def gkr_round(s, kind, eq4, num, den, n_vars, r, lam):
    """Out of place: the layer has 2^(n_vars + 2) values, the folded columns half that."""
    L = _L()
    half = 1 << (n_vars + 1)
    res = s.buf(8)
    od = [s.buf(half, kind="m31") for _ in range(4)]
    on = [s.buf(half, kind="m31") for _ in range(4)] if num else []

    def model(S):
        lay = _model_layer(S, kind, num, den)
        folded = {"kind": GM.GENERIC if kind == GM.MULT else kind,
                  "num": GM.fix_first_variable(lay["num"], r) if lay["num"] is not None else None,
                  "den": GM.fix_first_variable(lay["den"], r)}
        f0, f2 = GM.sum_f0_f2(folded, np.stack([S[x] for x in eq4]).astype(np.uint64), n_vars, lam)
        out = {res: np.array(tuple(f0) + tuple(f2), dtype=np.uint32)}
        out.update(zip(od, coords(folded["den"])))
        if on:
            out.update(zip(on, coords(folded["num"])))
        return out
    s.add(Op("tstwo_gkr_round", eq4 + (num or []) + den, [res] + od + on,
             lambda A: _call("tstwo_gkr_round", kind, _p4(A, eq4), _num_p4(A, kind, num), _p4(A, den), _p4(A, on) if on else L.p4([0] * 4),
                             _p4(A, od), n_vars, L.u32x(r), L.u32x(lam), C.c_void_p(A(res))),
             model, scratch="gkr ticket and slab"))
    return res, on, od


def mle_fix_first_variable(s, ins, log_n, r):
    """ins: one base column or four secure ones."""
    L = _L()
    o4 = [s.buf(1 << (log_n - 1), kind="m31") for _ in range(4)]
    if len(ins) == 1:
        s.add(Op("tstwo_mle_fix_first_variable_base", ins, o4,
                 lambda A: _call("tstwo_mle_fix_first_variable_base", C.c_void_p(A(ins[0])), log_n, L.u32x(r), _p4(A, o4)),
                 lambda S: dict(zip(o4, coords(GM.fix_first_variable(S[ins[0]].astype(np.uint64), r))))))
    else:
        s.add(Op("tstwo_mle_fix_first_variable_secure", ins, o4,
                 lambda A: _call("tstwo_mle_fix_first_variable_secure", _p4(A, ins), log_n, L.u32x(r), _p4(A, o4)),
                 lambda S: dict(zip(o4, coords(GM.fix_first_variable(np.stack([S[x] for x in ins]).astype(np.uint64), r))))))
    return o4


# ---- AIR and LogUp
def _felt(rng):
    return tuple(int(v) for v in rng.integers(0, P, size=4))


def air_wide_fib_trace(s, a, b, log, n_cols):
    cols = [s.buf(1 << log, kind="m31") for _ in range(n_cols)]
    s.add(Op("tstwo_air_wide_fib_trace", [a, b], cols,
             lambda A: _call("tstwo_air_wide_fib_trace", C.c_void_p(A(a)), C.c_void_p(A(b)), log, _ptrs(A, cols), n_cols),
             lambda S: dict(zip(cols, [w.astype(np.uint32) for w in AM.wide_fib_trace(S[a].astype(np.uint64), S[b].astype(np.uint64), n_cols)])),
             capturable=n_cols <= 64))
    return cols


def air_constraint_quotients(s, kind, cols, log, acc4, seed=0):
    """log_expand 1; cols hold 2^(log + 1) words; acc4 is added to, in place."""
    L = _L()
    rng = np.random.default_rng(9100 + seed)
    coeffs = [_felt(rng) for _ in range(AM.n_constraints(kind, len(cols)))]
    dinv = AM.denom_inv(log, log + 1)
    model = lambda S: dict(zip(acc4, coords(AM.quotients_on_domain(kind, [S[c].astype(np.uint64) for c in cols], log, 1, coeffs, dinv,
                                                                    np.stack([S[x] for x in acc4]).astype(np.uint64)))))
    s.add(Op("tstwo_air_constraint_quotients", cols + acc4, acc4,
             lambda A: _call("tstwo_air_constraint_quotients", 1 if kind == AM.MUL_ADD else 0, _ptrs(A, cols), len(cols), log, 1,
                             L.u32x([w for c in coeffs for w in c]), len(coeffs), L.u32x([int(d) for d in dinv]), _p4(A, acc4)),
             model, capturable=len(cols) <= 64))
    return acc4


def air_eval_program(s, cols, log, acc4, seed=0):
    L = _L()
    rng = np.random.default_rng(9200 + seed)
    n_constraints = 5
    words = XM.random_program(rng, len(cols), n_constraints, 40, max_offset=3)
    coeffs = [_felt(rng) for _ in range(n_constraints)]
    dinv = AM.denom_inv(log, log + 1)
    model = lambda S: dict(zip(acc4, coords(XM.eval_program_on_domain(words, [S[c].astype(np.uint64) for c in cols], log, 1, coeffs, dinv,
                                                                      np.stack([S[x] for x in acc4]).astype(np.uint64)))))
    s.add(Op("tstwo_air_eval_program", cols + acc4, acc4,
             lambda A: _call("tstwo_air_eval_program", _ptrs(A, cols), len(cols), log, 1, L.u32x(words), len(words) // 2,
                             L.u32x([w for c in coeffs for w in c]), n_constraints, L.u32x([int(d) for d in dinv]), _p4(A, acc4)),
             model, capturable=False, scratch="air program"))
    return acc4


def logup_column(s, fracs, prev4, log, seed=0):
    """fracs = [(term columns, numerator column or None)]; coefficients and constants are drawn here.  Denominators are
    random QM31 combinations: zero with probability 2^-124."""
    L = _L()
    rng = np.random.default_rng(9300 + seed)
    n = 1 << log
    spec = [(terms, num, [_felt(rng) for _ in terms], _felt(rng), int(rng.integers(1, P))) for terms, num in fracs]
    o4 = [s.buf(n, kind="m31") for _ in range(4)]
    reads = [t for terms, num, *_ in spec for t in terms] + [num for _, num, *_ in spec if num] + (prev4 or [])

    def model(S):
        ms = []
        for terms, num, coeffs, const, num_const in spec:
            den = np.zeros((4, n), dtype=np.uint64)
            for j in range(4):
                den[j] = const[j]
                for t, co in zip(terms, coeffs):
                    den[j] = (den[j] + co[j] * S[t].astype(np.uint64)) % P
            ms.append((S[num].astype(np.uint64) if num else np.full(n, num_const, dtype=np.uint64), den))
        prev = np.stack([S[x] for x in prev4]).astype(np.uint64) if prev4 else None
        return dict(zip(o4, coords(LM.column(ms, prev, n))))

    def call(A):
        descs, keep = (L.LogupFrac * len(spec))(), []
        for f, (terms, num, coeffs, const, num_const) in enumerate(spec):
            tab, cw = _ptrs(A, terms), L.u32x([w for co in coeffs for w in co])
            keep += [tab, cw]
            d = descs[f]
            d.cols, d.coeffs, d.n_terms = C.cast(tab, C.POINTER(L.vp)), C.cast(cw, L.u32p), len(terms)
            d.constant[:] = list(const)
            d.num, d.num_const = (A(num) if num else None), (0 if num else num_const)
        _call("tstwo_logup_column", descs, len(spec), _p4(A, prev4) if prev4 else None, log, _p4(A, o4))
    s.add(Op("tstwo_logup_column", reads, o4, call, model, capturable=False, scratch="logup descriptors"))
    return o4


# ---- context.hip
def copy(s, src, dst=None):
    n = s.sizes[src]
    dst = dst or s.buf(n, kind=s.kind[src])
    s.add(Op("tstwo_copy", [src], [dst], lambda A: _call("tstwo_copy", C.c_void_p(A(dst)), C.c_void_p(A(src)), 4 * n), lambda S: {dst: S[src].copy()}))
    return dst


def zero(s, n_words):
    dst = s.buf(n_words, kind="m31")
    s.add(Op("tstwo_zero", [], [dst], lambda A: _call("tstwo_zero", C.c_void_p(A(dst)), 4 * n_words), lambda S: {dst: np.zeros(n_words, dtype=np.uint32)}))
    return dst


def upload(s, words):
    """tstwo_upload of at most 16 KiB: the ring."""
    words = u32(words).copy()
    assert words.nbytes <= 16384
    dst = s.buf(words.size, kind="m31")
    s.add(Op("tstwo_upload", [], [dst], lambda A: _call("tstwo_upload", C.c_void_p(A(dst)), words.ctypes.data_as(C.c_void_p), words.nbytes),
             lambda S: {dst: words}, capturable=False))
    return dst


# ------------------------------------------------------------------ sequences
def rand_cols(s, rng, k, n, nonzero=False):
    return s.inputs([rng.integers(1 if nonzero else 0, P, size=n, dtype=np.uint32) for _ in range(k)])


class _Pool:
    """Columns of canonical M31 words by length, inputs and the outputs of earlier ops: where later ops take their operands."""

    def __init__(self, s, rng):
        self.s, self.rng, self.by_n = s, rng, {}

    def put(self, names):
        for x in names:
            self.by_n.setdefault(self.s.sizes[x], []).append(x)

    def take(self, k, n):
        """k distinct columns of n words: those an earlier op left where there are enough (two times in three), else fresh inputs."""
        have = self.by_n.get(n, [])
        if len(have) >= k and self.rng.integers(3) < 2:
            return [have[i] for i in sorted(self.rng.choice(len(have), size=k, replace=False))]
        fresh = rand_cols(self.s, self.rng, k, n)
        self.put(fresh)
        return fresh

    def own(self, k, n):
        """Columns an in-place op may overwrite: copies (tstwo_copy, an op of the sequence) of k pool columns, so that what the
        pool column held stays checked; beyond 8 columns fresh inputs that nothing else reads."""
        if k > 8:
            return rand_cols(self.s, self.rng, k, n)
        return [copy(self.s, x) for x in self.take(k, n)]


def scratch_tour(s, rng, pool=None, seed=0):
    """Quotient blob, AIR program, LogUp descriptors, GKR sum, GKR eq tables, quotient blob: the users that store different
    layouts at the same scratch offsets, back to back."""
    pool = pool or _Pool(s, rng)
    outs = []
    cols = pool.take(3, 1 << 6)
    outs += quotients_async(s, cols, 6, 2, samples=False, seed=seed)
    acc = pool.own(4, 1 << 6)
    air_eval_program(s, pool.take(6, 1 << 6), 5, acc, seed=seed)
    outs += logup_column(s, [(pool.take(2, 1 << 6), pool.take(1, 1 << 6)[0]), (pool.take(1, 1 << 6), None)], pool.take(4, 1 << 6), 6, seed=seed)
    kind = [GM.GP, GM.GENERIC, GM.MULT, GM.SINGLES][seed % 4]
    n_vars = 5
    num, den = gkr_layer_inputs(s, rng, kind, n_vars + 1)
    eq4 = gkr_gen_eq_evals(s, [GM.random_felt(rng) for _ in range(n_vars - 1)], GM.random_felt(rng))
    gkr_sum_poly_async(s, kind, eq4, num, den, n_vars, GM.random_felt(rng))
    outs += quotients_async(s, pool.take(5, 1 << 6), 6, 3, samples=True, seed=seed + 1)
    pool.put(outs + acc)
    return pool


def _makers():
    """name -> function(s, rng, pool) adding one catalogue op (with the copies an in-place op needs in front of it)."""
    M = {}
    logs = (5, 6, 7, 9, 10)
    lg = lambda rng: int(rng.choice(logs))

    def reg(f):
        M[f.__name__] = f
        return f

    @reg
    def m31(s, rng, pool):
        n = (1 << lg(rng)) - int(rng.integers(0, 2)) * 3            # ragged lengths take the scalar tail
        op = ["add", "sub", "mul", "neg"][int(rng.integers(4))]
        a, b = pool.take(2, n)
        pool.put([m31_op(s, op, a, None if op == "neg" else b)])

    @reg
    def qmul(s, rng, pool):
        n = 1 << lg(rng)
        pool.put(qm31_mul(s, pool.take(4, n), pool.take(4, n)))

    @reg
    def accumulate(s, rng, pool):
        n = 1 << lg(rng)
        pool.put(secure_accumulate(s, pool.own(4, n), pool.take(4, n)))

    @reg
    def bitrev(s, rng, pool):
        log = int(rng.choice((5, 9, 12, 13)))                       # tiled from log 12
        pool.put(bit_reverse(s, pool.own(int(rng.integers(1, 4)), 1 << log)))

    @reg
    def inverse(s, rng, pool):
        k = (1, 2, 4)[int(rng.integers(3))]
        pool.put(batch_inverse_async(s, rand_cols(s, rng, k, 1 << lg(rng), nonzero=True)))

    @reg
    def transform(s, rng, pool):
        log = int(rng.choice((5, 6, 8, 12, 13)))
        pool.put(cfft(s, ["evaluate", "interpolate"][int(rng.integers(2))], pool.own(int(rng.integers(1, 5)), 1 << log), log))

    @reg
    def transform_wide(s, rng, pool):
        k = (65, 70)[int(rng.integers(2))]
        pool.put(cfft(s, ["evaluate", "interpolate"][int(rng.integers(2))], pool.own(k, 1 << 6), 6))

    @reg
    def interpolate_to(s, rng, pool):
        k = (3, 65)[int(rng.integers(2))]
        log = 6 if k > 64 else lg(rng)
        pool.put(cfft_interpolate_to(s, pool.take(k, 1 << log), log))

    @reg
    def extend(s, rng, pool):
        log = lg(rng)
        pool.put([poly_extend(s, pool.take(1, 1 << log)[0], log, log + int(rng.integers(0, 3)))])

    @reg
    def evaluate_extended(s, rng, pool):
        k = (2, 65)[int(rng.integers(2))]
        log = 6 if k > 64 else lg(rng)
        pool.put(cfft_evaluate_extended(s, pool.take(k, 1 << (log - 1)), log - 1, log))

    @reg
    def line_fold(s, rng, pool):
        k = lg(rng)
        entry = ["dev", "tw", "rows"][int(rng.integers(3))]
        pool.put(fold_line(s, entry, pool.take(4, 1 << k), k, rows=(4, (1 << (k - 1)) - 8)))

    @reg
    def circle_fold(s, rng, pool):
        n = lg(rng)
        entry = ["dev", "tw", "rows"][int(rng.integers(3))]
        pool.put(fold_circle_into_line(s, entry, pool.own(4, 1 << (n - 1)), pool.take(4, 1 << n), n, rows=(4, (1 << (n - 1)) - 8)))

    @reg
    def merkle(s, rng, pool):
        which = int(rng.integers(4))
        log = int(rng.choice((5, 6, 9)))
        if which == 0:
            merkle_commit(s, pool.take(3, 1 << log) + pool.take(2, 1 << 5), [log] * 3 + [5] * 2)
        elif which == 1:
            merkle_commit_many(s, [(pool.take(3, 1 << log), [log] * 3), (pool.take(17, 1 << 5), [5] * 17)])
        elif which == 2:
            prev = merkle_commit_layer(s, log, None, pool.take(2, 1 << log))
            merkle_commit_layer(s, log - 1, prev, pool.take(17, 1 << (log - 1)))
        else:
            poseidon_commit(s, pool.take(3, 1 << 5), 5)

    @reg
    def quotients(s, rng, pool):
        pool.put(quotients_async(s, pool.take(int(rng.integers(1, 6)), 1 << 6), 6, int(rng.integers(1, 5)), bool(rng.integers(2)),
                                 seed=int(rng.integers(1000))))

    @reg
    def gkr(s, rng, pool):
        kind = [GM.GP, GM.GENERIC, GM.MULT, GM.SINGLES][int(rng.integers(4))]
        n_vars = int(rng.choice((4, 5, 9)))
        which = int(rng.integers(4))
        lam, r = GM.random_felt(rng), GM.random_felt(rng)
        if which == 0:
            num, den = gkr_layer_inputs(s, rng, kind, n_vars + 1)
            on, od = gkr_next_layer(s, kind, num, den, n_vars + 1)
            pool.put((on or []) + od)
        elif which == 1:
            num, den = gkr_layer_inputs(s, rng, kind, n_vars + 1)
            gkr_sum_poly_async(s, kind, pool.take(4, 1 << (n_vars - 1)), num, den, n_vars, lam)
        elif which == 2:
            num, den = gkr_layer_inputs(s, rng, kind, n_vars + 2)
            eq4 = gkr_gen_eq_evals(s, [GM.random_felt(rng) for _ in range(n_vars - 1)], GM.random_felt(rng))
            _, on, od = gkr_round(s, kind, eq4, num, den, n_vars, r, lam)
            pool.put(on + od)
        else:
            k = (1, 4)[int(rng.integers(2))]
            pool.put(mle_fix_first_variable(s, pool.take(k, 1 << n_vars), n_vars, r))

    @reg
    def air(s, rng, pool):
        which, log = int(rng.integers(3)), int(rng.choice((5, 6, 9)))
        if which == 0:
            a, b = pool.take(2, 1 << log)
            pool.put(air_wide_fib_trace(s, a, b, log, (3, 17, 70)[int(rng.integers(3))] if log == 6 else 3))
        elif which == 1:
            kind, k = [(AM.WIDE_FIB, 4), (AM.MUL_ADD, 3)][int(rng.integers(2))]
            pool.put(air_constraint_quotients(s, kind, pool.take(k, 2 << log), log, pool.own(4, 2 << log), seed=int(rng.integers(1000))))
        else:
            pool.put(air_eval_program(s, pool.take(6, 2 << log), log, pool.own(4, 2 << log), seed=int(rng.integers(1000))))

    @reg
    def logup(s, rng, pool):
        log = int(rng.choice((5, 6, 10)))
        n = 1 << log
        fr = [(pool.take(int(rng.integers(1, 4)), n), pool.take(1, n)[0] if rng.integers(2) else None) for _ in range(int(rng.integers(1, 4)))]
        pool.put(logup_column(s, fr, pool.take(4, n) if rng.integers(2) else None, log, seed=int(rng.integers(1000))))

    @reg
    def plumbing(s, rng, pool):
        which, n = int(rng.integers(3)), 1 << lg(rng)
        if which == 0:
            pool.put([copy(s, pool.take(1, n)[0])])
        elif which == 1:
            pool.put([zero(s, n)])
        else:
            pool.put([upload(s, rng.integers(0, P, size=min(n, 4096), dtype=np.uint32))])
    return M


MAKERS = _makers()


# makers whose ops never go through the upload ring: at most 64 columns, no host-array blob
RING_FREE = ("accumulate", "bitrev", "circle_fold", "extend", "gkr", "inverse", "line_fold", "m31", "merkle", "qmul", "transform")


def random_sequence(seed, n_ops=40, tour=True, ring_free=False):
    """A seeded sequence of about n_ops catalogue ops with chained buffers (not counting the copies in front of in-place ops).  tour:
    starts with scratch_tour(), so that every seed holds each pair of scratch users with different layouts back to back.
    ring_free: behind the tour only ops that upload nothing through the ring (for runs behind a plug: the 17th ring upload behind
    pending work makes the host wait for the 1st)."""
    rng = np.random.default_rng(seed)
    s = Seq()
    pool = _Pool(s, rng)
    if tour:
        scratch_tour(s, rng, pool, seed=seed)
    names = sorted(RING_FREE if ring_free else MAKERS)
    while sum(op.entry != "tstwo_copy" for op in s.ops) < n_ops:
        before = len(s.ops)
        MAKERS[names[int(rng.integers(len(names)))]](s, rng, pool)
        assert not ring_free or all(op.capturable for op in s.ops[before:])
    return s


def capturable_sequence(data_seed):
    """One op of every capturable catalogue entry (no host-array upload: at most 64 columns, no quotient, AIR program, LogUp or
    tstwo_upload call), chained where the shapes allow.  The STRUCTURE and every by-value scalar are fixed; only the words of the
    input buffers depend on data_seed, so that one captured graph serves every data_seed."""
    s = Seq()
    rng = np.random.default_rng(10_000 + data_seed)            # input words
    fix = np.random.default_rng(77)                            # scalars recorded by value
    felt = lambda: GM.random_felt(fix)
    c = lambda k, n, nz=False: rand_cols(s, rng, k, n, nz)
    a, b = c(2, 1 << 9)
    t = m31_op(s, "add", a, b); t = m31_op(s, "mul", t, a); t = m31_op(s, "sub", t, b); t = m31_op(s, "neg", t)
    q = qm31_mul(s, c(4, 1 << 7), c(4, 1 << 7))
    secure_accumulate(s, q, c(4, 1 << 7))
    bit_reverse(s, [copy(s, t)] + c(2, 1 << 9))
    bit_reverse(s, c(1, 1 << 12))
    batch_inverse_async(s, c(1, 1 << 9, True)); batch_inverse_async(s, c(2, 1 << 9, True)); batch_inverse_async(s, c(4, 1 << 9, True))
    ext = poly_extend(s, c(1, 1 << 5)[0], 5, 7)
    ev = cfft(s, "evaluate", [ext] + c(3, 1 << 7), 7)                       # evaluate ...
    merkle_commit(s, ev, [7] * 4)                                           # ... commit ...
    line = fold_circle_into_line(s, "tw", [zero(s, 1 << 6) for _ in range(4)], ev, 7)     # ... fold, no host step between
    fold_line(s, "tw", line, 6)
    fold_line(s, "dev", c(4, 1 << 6), 6)
    fold_line(s, "rows", c(4, 1 << 6), 6, rows=(4, 8))
    fold_circle_into_line(s, "dev", c(4, 1 << 5), c(4, 1 << 6), 6)
    fold_circle_into_line(s, "rows", c(4, 1 << 5), c(4, 1 << 6), 6, rows=(8, 16))
    co = cfft_interpolate_to(s, ev, 7)
    cfft(s, "interpolate", c(2, 1 << 12), 12)
    cfft_evaluate_extended(s, co[:2], 7, 8)
    merkle_commit_many(s, [(c(3, 1 << 6), [6] * 3), (c(17, 1 << 5), [5] * 17)])
    prev = merkle_commit_layer(s, 6, None, c(2, 1 << 6))
    merkle_commit_layer(s, 5, prev, c(17, 1 << 5))
    poseidon_commit(s, c(3, 1 << 5), 5)
    for kind in (GM.GP, GM.GENERIC, GM.MULT, GM.SINGLES):
        n_vars = 5
        num, den = gkr_layer_inputs(s, rng, kind, n_vars + 2)
        on, od = gkr_next_layer(s, kind, num, den, n_vars + 2)              # a layer of 2^(n_vars + 1) values
        k2 = GM.GP if kind == GM.GP else GM.GENERIC
        eq4 = gkr_gen_eq_evals(s, [felt() for _ in range(n_vars - 1)], felt())
        gkr_sum_poly_async(s, k2, eq4, on, od, n_vars, felt())
        gkr_round(s, kind, eq4[:], num, den, n_vars, felt(), felt())
    mle_fix_first_variable(s, c(1, 1 << 6), 6, felt())
    mle_fix_first_variable(s, c(4, 1 << 6), 6, felt())
    tr = air_wide_fib_trace(s, *c(2, 1 << 6), 5 + 1, 4)
    air_constraint_quotients(s, AM.WIDE_FIB, tr, 5, c(4, 1 << 6), seed=1)
    assert all(op.capturable for op in s.ops)
    return s
