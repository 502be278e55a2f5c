"""-m gpu call-sequence tests: the state the library keeps BETWEEN calls (tests/sequence.py has the ops, references, runner, plug).

Every other GPU test runs one entry point alone.  Here calls are enqueued back to back with nothing between them that
synchronises, often behind a plug that keeps the stream busy, so that a wrong cache hit, a staging slot rewritten early, a stale
ticket or flag, a recycled block written too soon or a graph holding an address the library no longer owns is a wrong word and
not a race won by luck.  Shared state -> test: scratch block: (1), (5), (8), (9); upload ring: (2), (7); pointer-table slots and
their cache: (3); result page and pinned block: (3), (7); zero flag: (6), (8); sequence word: every download here; allocator:
(4); copy streams: (7); tstwo_set_stream: (7); tstwo_graph_*: (8), (9).
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import rand_column
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

from tstwo_amd import _lib as L  # noqa: E402
import sequence as SQ  # noqa: E402

vp = C.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _init():
    L.init(0)
    yield
    L.sync()


@pytest.fixture(scope="module")
def plug():
    p = SQ.Plug()
    p.enqueue(); p.host_done(); L.sync()           # once without a check: the first launches load the transform's code objects
    yield p
    L.sync()
    p.free()


# ------------------------------------------------------------------ (1) random interleavings
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_interleaving(seed):
    """About 40 catalogue ops (plus the copies in front of in-place ones) with chained buffers, every buffer checked.  Each seed
    starts with the scratch tour: quotient blob, AIR program, LogUp descriptors, GKR eq tables, GKR ticket and slab, quotient blob."""
    SQ.run(SQ.random_sequence(seed))


@pytest.mark.parametrize("seed", [4, 5])
def test_random_interleaving_behind_a_plug(seed, plug):
    """The same with a plug in front.  The ops behind the tour are those that upload nothing through the ring: the 17th ring upload
    behind a running plug waits for the 1st (test (2) is about that), and a host that waits cannot run ahead."""
    s = SQ.random_sequence(seed, ring_free=True)
    assert sum(op.scratch is not None for op in s.ops) >= 6
    _, ratio = SQ.run(s, plug)
    print(f"plug ratio {ratio:.1f}")


# ------------------------------------------------------------------ (2) the upload ring wraps behind a plug
def ring_wrap(plug):
    """40 uploads of 16 KiB of distinct words into distinct buffers behind a plug: two and a half trips round the 16 slots while the
    first copies still wait.  The first 16 uploads find free slots and must return while the plug runs -- that is the precondition;
    from the 17th on the library has to wait for a slot's copy, so those calls last as long as the plug does."""
    n_up, words = 40, 4096
    data = [np.random.default_rng(500 + i).integers(0, 1 << 32, size=words, dtype=np.uint32) for i in range(n_up)]
    dst = L.DeviceBuffer(4 * words * n_up)
    try:
        dst.zero()
        L.sync()
        plug.enqueue()
        for i in range(n_up):
            L.call("tstwo_upload", vp(dst.ptr + 4 * words * i), data[i].ctypes.data_as(vp), 4 * words)
            if i == 15:
                plug.host_done()
            if i == 16:
                t_wrap = time.perf_counter()
        got = dst.download()
        ratio = plug.check()
    finally:
        dst.free()
    for i in range(n_up):
        bad = np.flatnonzero(got[i * words:(i + 1) * words] != data[i])
        assert bad.size == 0, f"upload #{i}: first differing word {int(bad[0])}, last {int(bad[-1])} (slot {i % 16})"
    # the wrap itself: upload #16 reuses slot 0, whose copy waits behind the plug, so the call cannot return before the plug has
    # ended, and the plug ends no sooner than its device time after the host began to enqueue it
    wrap_ms = 1e3 * (t_wrap - plug.t0)
    assert wrap_ms >= plug.device_ms, f"upload #16 returned {wrap_ms:.2f} ms after the plug was enqueued, the plug ran {plug.device_ms:.2f} ms: " \
                                      "slot 0 was rewritten while its first copy was still pending"
    return got, ratio


def test_upload_ring_wrap_behind_a_plug(plug):
    _, ratio = ring_wrap(plug)
    print(f"plug ratio {ratio:.1f}")


# ------------------------------------------------------------------ (3) pointer-table slots and their host cache
def _sample_point():
    return SQ._sample_points(1)[0]


def table_sequences():
    """Part one: A (65 columns), B with one pointer changed, B with all changed, A again, interpolate_to whose src table is the
    table A left in slot 0, a 70-column call.  Part two, behind a tstwo_eval_at_point_batch over the 65 coefficient columns (it
    puts their table into slot 0): a transform of those same columns (a hit on what eval_at_point left), and A's columns again."""
    s = SQ.Seq()
    rng = np.random.default_rng(33)
    X, W, V = SQ.rand_cols(s, rng, 65, 64), SQ.rand_cols(s, rng, 65, 64), SQ.rand_cols(s, rng, 70, 64)
    z = SQ.rand_cols(s, rng, 1, 64)
    SQ.cfft(s, "evaluate", X, 6)
    SQ.cfft(s, "evaluate", X[:64] + z, 6)
    SQ.cfft(s, "evaluate", W, 6)
    SQ.cfft(s, "interpolate", X, 6)
    D = SQ.cfft_interpolate_to(s, X, 6)
    SQ.cfft(s, "interpolate", V, 6)
    n1 = len(s.ops)
    SQ.cfft(s, "evaluate", D, 6)
    SQ.cfft(s, "evaluate", X, 6)
    return s, n1, D


@pytest.mark.parametrize("plugged", [False, True], ids=["plain", "plug"])
def test_pointer_table_slots(plugged, request):
    plug = request.getfixturevalue("plug") if plugged else None
    s, n1, D = table_sequences()
    want = s.expected()
    px, py = _sample_point()
    state1 = s.initial_state()
    for op in s.ops[:n1]:
        state1.update(op.expected(state1))
    arena = SQ.Arena(s)
    try:
        L.sync()
        if plug:
            plug.enqueue()
        SQ.enqueue_all(s, arena.addr, s.ops[:n1])
        if plug:
            plug.host_done()
        out = (C.c_uint32 * (4 * len(D)))()
        L.call("tstwo_eval_at_point_batch", L.ptr_array([arena.addr(d) for d in D]), len(D), 6, L.u32x(px), L.u32x(py), out)
        SQ.enqueue_all(s, arena.addr, s.ops[n1:])
        got = arena.download()
        if plug:
            print(f"plug ratio {plug.check():.1f}")
    finally:
        arena.free()
    msgs = SQ.compare(s, got, want)
    wrong = [i for i, d in enumerate(D) if tuple(out[4 * i:4 * i + 4]) != orc.eval_at_point(state1[d], 6, px, py)]
    if wrong:
        msgs.append(f"tstwo_eval_at_point_batch: {len(wrong)} of {len(D)} columns differ, first {wrong[0]}, last {wrong[-1]}")
    assert not msgs, f"{len(msgs)} differences; " + "; ".join(msgs[:6])


# ------------------------------------------------------------------ (4) allocator recycling
def _process_alloc_mode():
    """The mode the library takes from the environment at its first tstwo_malloc (context.hip, probe_env): what the process ran
    in before a test set a mode of its own.  The library has no call that reads the mode back."""
    env = os.environ
    kind = env.get("TSTWO_ALLOC")
    if kind == "direct" or (kind != "async" and "TSTWO_NO_POOL" in env):
        base = L.ALLOC_DIRECT
    else:
        base = L.ALLOC_ASYNC if kind == "async" else L.ALLOC_POOL
    return base | (L.ALLOC_POISON if env.get("TSTWO_POISON", "0") not in ("", "0") else 0)


@pytest.mark.parametrize("poison", [False, True], ids=["pool", "poison"])
def test_allocator_recycles_a_block_an_enqueued_kernel_still_reads(poison, plug):
    """Behind a plug: a kernel that reads X is enqueued, X is freed, a block of the same class is allocated (the same pointer: the
    condition of the test) and a writer into it is enqueued.  The reader must have seen X's words, the new block must end with the
    writer's; with POISON the 0xA5 fill of the new block must be ordered behind the reader too."""
    n = 3 << 18                                         # 3 MiB: the 1.5 * 2^21 class, which nothing else here uses
    x, y, w = rand_column(41, n), rand_column(42, n), rand_column(43, n)
    L.call("tstwo_set_alloc_mode", L.ALLOC_POOL | (L.ALLOC_POISON if poison else 0))
    bufs = []
    try:
        bufs = [L.DeviceBuffer(4 * n) for _ in range(4)]
        bx, by, bw, bo = bufs
        for b, a in ((bx, x), (by, y), (bw, w)):
            b.upload(a)
        L.sync()
        old = bx.ptr
        plug.enqueue()
        L.call("tstwo_m31_add", vp(bx.ptr), vp(by.ptr), vp(bo.ptr), n)          # the reader
        bx.free()
        bn = L.DeviceBuffer(4 * n)
        bufs.append(bn)
        same = bn.ptr == old
        L.call("tstwo_copy", vp(bn.ptr), vp(bw.ptr), 4 * n)                       # the writer
        plug.host_done()
        got_o, got_n = bo.download(), bn.download()
        ratio = plug.check()
    finally:
        for b in bufs:
            b.free()                                    # (a freed buffer's free() does nothing)
        L.call("tstwo_set_alloc_mode", _process_alloc_mode())
    assert same, "tstwo_malloc did not hand the freed block out again: the test needs the recycled pointer"
    print(f"plug ratio {ratio:.1f}")
    bad = np.flatnonzero(got_o != orc.col_op("add", x, y))
    assert bad.size == 0, f"the reader saw other words than X held: first differing word {int(bad[0])} ({int(got_o[bad[0]]):#x}), last {int(bad[-1])}"
    assert (got_n == w).all()


# ------------------------------------------------------------------ (5), (9) scratch growth, in a fresh process
_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import ctypes as C
import numpy as np
from tstwo_amd import _lib as L
import sequence as SQ
import gkr_model as GM
mode = sys.argv[1]
L.init(0)

def tour(seed):
    s = SQ.Seq()
    SQ.scratch_tour(s, np.random.default_rng(seed), seed=seed)
    SQ.run(s)

def gather_2_16(before_call=None):
    # 2^16 one-word items: 16 B x 65536 request items + 4 B x 65536 result words = 1.25 MiB of scratch, the cheapest call that
    # outgrows the initial 1 MiB block; nothing before it in this process asks for more than a few KiB.  before_call() runs when
    # the arguments are ready, right in front of the library call.
    n = 1 << 16
    src = np.random.default_rng(5).integers(0, 1 << 32, size=1 << 12, dtype=np.uint32)
    buf = L.DeviceBuffer(src.nbytes); buf.upload(src)
    idx = np.random.default_rng(6).integers(0, src.size, size=n, dtype=np.uint64)
    out = np.empty(n, dtype=np.uint32)
    srcs = (L.vp * n)(*([buf.ptr] * n))
    if before_call:
        before_call()
    L.call("tstwo_gather_words", srcs, idx.ctypes.data_as(C.POINTER(C.c_uint64)), 1, n, out.ctypes.data_as(L.u32p))
    assert (out == src[idx]).all(), "gather of 2^16 items"
    buf.free()

def gkr_sequence(data_seed):
    s = SQ.Seq()
    rng, fix = np.random.default_rng(300 + data_seed), np.random.default_rng(9)
    for kind in (GM.GP, GM.GENERIC, GM.MULT, GM.SINGLES):
        n_vars = 6
        num, den = SQ.gkr_layer_inputs(s, rng, kind, n_vars + 2)
        eq4 = SQ.gkr_gen_eq_evals(s, [GM.random_felt(fix) for _ in range(n_vars - 1)], GM.random_felt(fix))
        _, on, od = SQ.gkr_round(s, kind, eq4, num, den, n_vars, GM.random_felt(fix), GM.random_felt(fix))
        SQ.gkr_sum_poly_async(s, GM.GP if kind == GM.GP else (GM.SINGLES if kind == GM.SINGLES else GM.GENERIC), eq4, on or None, od, n_vars, GM.random_felt(fix))
    return s

if mode == "growth":
    tour(1)
    plug = SQ.Plug()
    s = SQ.Seq()
    rng = np.random.default_rng(2)
    SQ.quotients_async(s, SQ.rand_cols(s, rng, 5, 64), 6, 3, samples=False)
    SQ.quotients_async(s, SQ.rand_cols(s, rng, 3, 64), 6, 2, samples=True)
    plug.enqueue(); plug.host_done(); L.sync()           # once unchecked: the first launches load the transform's code objects
    want = s.expected()
    arena = SQ.Arena(s)
    L.sync()
    # the block grows while its users are still in flight: the quotient kernels wait behind the plug with their blobs in the
    # 1 MiB block when the gather asks for 1.25 MiB, uploads its items and runs; the interval of the precondition ends in front
    # of the gather call, so the plug (and with it both quotient calls) was still pending when the library grew the block
    def enqueue_users():
        plug.enqueue()
        SQ.enqueue_all(s, arena.addr)
    gather_2_16(before_call=lambda: (enqueue_users(), plug.host_done()))
    got = arena.download()
    print("plug ratio %.1f (device %.1f ms, host %.2f ms)" % (plug.check(), plug.device_ms, plug.host_ms))
    msgs = SQ.compare(s, got, want)
    assert not msgs, "quotients in flight across the growth: " + "; ".join(msgs[:4])
    arena.free()
    tour(3)
    SQ.run(s)
    plug.free()
else:
    assert mode == "graph"
    seqs = [gkr_sequence(d) for d in range(3)]
    assert seqs[0].signature() == seqs[1].signature() and seqs[0].layout() == seqs[2].layout()
    arena = SQ.Arena(seqs[0])
    L.sync()
    SQ.enqueue_all(seqs[0], arena.addr)                  # eager: sizes the scratch for these calls
    msgs = SQ.compare(seqs[0], arena.download())
    assert not msgs, "eager: " + "; ".join(msgs[:4])
    L.call("tstwo_graph_begin_capture")
    h = C.c_void_p()
    try:
        SQ.enqueue_all(seqs[0], arena.addr)
    finally:
        L.call("tstwo_graph_end_capture", C.byref(h))
    staged = []
    for d in (1, 2):
        b = L.DeviceBuffer(arena.total); b.upload(seqs[d].image()); staged.append(b)
    L.sync()
    for step, d in enumerate((1, 2)):
        L.call("tstwo_copy", C.c_void_p(arena.buf.ptr), C.c_void_p(staged[step].ptr), arena.total)
        L.call("tstwo_graph_launch", h)
        msgs = SQ.compare(seqs[d], arena.download())
        assert not msgs, ("replay %d: " % step) + "; ".join(msgs[:4])
        if step == 0:
            # a captured call that would have to GROW the scratch is refused and records nothing: a quotient call whose blob of
            # 2^17 + 8 column pointers (all the same column) exceeds the 1 MiB block
            n = (1 << 17) + 8
            L.call("tstwo_graph_begin_capture")
            h2, raised = C.c_void_p(), None
            try:
                L.call("tstwo_quotients_accumulate_async", SQ.half_odds(5), 6, (L.vp * n)(*([arena.buf.ptr] * n)), n, 1, L.u32x([0, 1]),
                       L.u32x([0]), L.u32x([1] * 12), L.u32x([1, 0, 0, 0]), L.u32x([1, 2]), L.u32x([3, 4]), L.u32x([5, 6]), L.u32x([7, 8]),
                       L.p4([staged[1].ptr + 256 * k for k in range(4)]))
            except L.TstwoError as e:
                raised = e
            finally:
                try:
                    L.call("tstwo_graph_end_capture", C.byref(h2))
                except L.TstwoError:
                    pass
                if h2.value:
                    L.call("tstwo_graph_destroy", h2)
            assert raised is not None and raised.code == 7 and "scratch growth during graph capture" in str(raised), raised
            gather_2_16()                               # the scratch block grows: the graph keeps the retired one
            tour(4)                                      # and eager users now share the new one
    L.call("tstwo_graph_destroy", h)
L.sync()
print("sequence child ok")
"""


def _child(mode):
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    script = _CHILD.format(root=os.path.dirname(tests_dir), tests=tests_dir)
    out = subprocess.run([sys.executable, "-c", script, mode], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("sequence child ok"), out.stdout[-1500:]
    return out.stdout


def test_scratch_growth_between_scratch_users():
    """In a fresh process, because the block never shrinks: the scratch tour; then a plug, two async quotient calls behind it and,
    while they are still pending (the plug's precondition, taken in front of the gather call), the 2^16-item tstwo_gather_words
    that outgrows the 1 MiB block (its own output checked); the quotient outputs must be the oracle's although the block their
    kernels read was outgrown before they ran.  Then the tour and the quotient calls again, on the new block."""
    print(_child("growth"))


def test_graph_replay_after_scratch_growth():
    """A graph of the GKR entry points (gen_eq_evals, round, sum_poly_async, all four kinds) records scratch addresses by value.
    Replay, the 2^16-item gather that makes the library outgrow its scratch block, replay again with new inputs: both replays must
    give the model's words.  The outgrown block is retired, not freed (include/tstwo_hip.h, "Rules while capturing").  In between,
    a captured call that would itself have to grow the block (a quotient call with a blob above 1 MiB) must be refused with
    "scratch growth during graph capture" and leave the stream usable."""
    _child("graph")


# ------------------------------------------------------------------ (6) the sticky zero flag
def _ten_unrelated_ops():
    s = SQ.Seq()
    rng = np.random.default_rng(66)
    c = lambda k, n: SQ.rand_cols(s, rng, k, n)
    a, b = c(2, 1000)
    t = SQ.m31_op(s, "mul", SQ.m31_op(s, "add", a, b), b)
    q = SQ.qm31_mul(s, c(4, 256), c(4, 256))
    SQ.secure_accumulate(s, q, c(4, 256))
    SQ.copy(s, t)
    ev = SQ.cfft(s, "evaluate", c(4, 1 << 7), 7)
    SQ.merkle_commit(s, ev, [7] * 4)
    SQ.fold_line(s, "tw", c(4, 1 << 6), 6)
    SQ.batch_inverse_async(s, SQ.rand_cols(s, rng, 4, 512, nonzero=True))        # a clean inverse must not clear the flag either
    SQ.zero(s, 300)
    assert len(s.ops) == 10
    return s


def test_zero_flag_is_sticky_across_unrelated_calls_and_raises_once():
    """The header: a zero input of an _async inverse "sets a sticky flag ... instead of failing the call (the affected outputs are
    unspecified)"; tstwo_check_zero_flag "synchronises ONCE, clears the flag and fails ... if any call since the last check met a
    zero".  Nothing is promised for the flagged call's outputs, its non-zero rows included, so nothing is asserted about them."""
    n = 1 << 10
    col = rand_column(61, n, nonzero=True)
    col[5] = 0
    bi, bo = L.DeviceBuffer(4 * n), L.DeviceBuffer(4 * n)
    bi.upload(col)
    s = _ten_unrelated_ops()
    want = s.expected()
    arena = SQ.Arena(s)
    try:
        L.sync()
        L.call("tstwo_check_zero_flag")                                           # clean before
        L.call("tstwo_m31_batch_inverse_async", vp(bi.ptr), vp(bo.ptr), n)
        SQ.enqueue_all(s, arena.addr)
        with pytest.raises(L.TstwoError, match="0 has no inverse") as e:
            L.call("tstwo_check_zero_flag")
        assert e.value.code == 2
        L.call("tstwo_check_zero_flag")                                           # raised once: cleared
        got = arena.download()
    finally:
        arena.free(); bi.free(); bo.free()
    msgs = SQ.compare(s, got, want)
    assert not msgs, "; ".join(msgs[:6])


def test_synchronous_inverse_reports_an_unchecked_flag_of_an_earlier_async_call():
    """The header: the synchronous inverses are "= async + check", and the check reports "any call since the last check".  So a
    synchronous inverse of a column WITHOUT zeros, called while an earlier _async call's flag is still unchecked, fails with "0 has
    no inverse" and clears the flag; its own outputs are the oracle's all the same, and the next check passes.  Code and header agree."""
    n = 1 << 10
    col, clean = rand_column(62, n, nonzero=True), rand_column(63, n, nonzero=True)
    col[n - 1] = 0
    bi, bo, ci, co = [L.DeviceBuffer(4 * n) for _ in range(4)]
    try:
        bi.upload(col); ci.upload(clean)
        L.call("tstwo_check_zero_flag")
        L.call("tstwo_m31_batch_inverse_async", vp(bi.ptr), vp(bo.ptr), n)
        with pytest.raises(L.TstwoError, match="0 has no inverse"):
            L.call("tstwo_m31_batch_inverse", vp(ci.ptr), vp(co.ptr), n)
        assert (co.download() == orc.m31_batch_inverse(clean)).all()
        L.call("tstwo_check_zero_flag")
        L.call("tstwo_m31_batch_inverse", vp(ci.ptr), vp(co.ptr), n)              # and the synchronous call works again
    finally:
        for b in (bi, bo, ci, co):
            b.free()


# ------------------------------------------------------------------ (7) a borrowed stream
def _on_current_stream(plug):
    """Sequence (1), the ring test (2), an upload_async / upload_fence pair in front of a kernel that reads the uploaded words, and
    a synchronous call that reads back through the result page.  Returns every downloaded word."""
    img, _ = SQ.run(SQ.random_sequence(1))
    ring, _ = ring_wrap(plug)
    n = 1 << 14
    a, b = rand_column(71, n), rand_column(72, n)
    pin = L.PinnedArray(n)
    pin.array[:] = a
    ba, bb, bo = [L.DeviceBuffer(4 * n) for _ in range(3)]
    bb.upload(b)
    ba.upload_async(pin.array)
    L.upload_fence()
    L.call("tstwo_m31_mul", vp(ba.ptr), vp(bb.ptr), vp(bo.ptr), n)
    prod = bo.download()
    assert (prod == orc.col_op("mul", a, b)).all()
    pieces = L.download_many([(bo.ptr, 1000), (bb.ptr + 4 * 17, 3), (ba.ptr, n // 2)])          # 36 KiB: the mapped result page
    assert (pieces[0] == prod[:1000]).all() and (pieces[1] == b[17:20]).all() and (pieces[2] == a[:n // 2]).all()
    L.upload_wait()
    pin.free()
    for x in (ba, bb, bo):
        x.free()
    return [img, ring, prod] + pieces


def test_borrowed_stream_gives_the_words_of_the_own_stream(plug):
    hip = C.CDLL("libamdhip64.so")
    stream = vp()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and stream.value           # 1 = hipStreamNonBlocking
    try:
        try:
            L.call("tstwo_set_stream", stream)
            borrowed = _on_current_stream(plug)
            L.sync()
        finally:
            L.call("tstwo_set_stream", None)
        own = _on_current_stream(plug)
    finally:
        L.sync()
        assert hip.hipStreamDestroy(stream) == 0
    assert len(own) == len(borrowed)
    for k, (x, y) in enumerate(zip(borrowed, own)):
        assert x.shape == y.shape and (x == y).all(), k


# ------------------------------------------------------------------ (8) graph replay beyond FRI
def _eager_state_rewriters(step):
    """Eager calls between replays that rewrite what a graph must not depend on: the scratch (quotient blob, gather items), the
    ring (blob, pointer table, gather items), table slot 0 (70 columns), the result page (gather), the zero flag."""
    s = SQ.Seq()
    rng = np.random.default_rng(800 + step)
    SQ.quotients_async(s, SQ.rand_cols(s, rng, 4, 64), 6, 2, samples=bool(step % 2), seed=step)
    SQ.cfft(s, "evaluate", SQ.rand_cols(s, rng, 70, 64), 6)
    SQ.run(s)
    src = rng.integers(0, 1 << 32, size=512, dtype=np.uint32)
    buf = L.DeviceBuffer(src.nbytes)
    buf.upload(src)
    idx = rng.integers(0, 512 // 8, size=33, dtype=np.uint64)
    out = np.empty(33 * 8, dtype=np.uint32)
    L.call("tstwo_gather_words", (vp * 33)(*([buf.ptr] * 33)), idx.ctypes.data_as(C.POINTER(C.c_uint64)), 8, 33, out.ctypes.data_as(L.u32p))
    assert (out.reshape(33, 8) == src.reshape(-1, 8)[idx]).all()
    zcol = np.zeros(64, dtype=np.uint32)
    buf.upload(zcol)
    L.call("tstwo_m31_batch_inverse_async", vp(buf.ptr), vp(buf.ptr + 1024), 64)
    with pytest.raises(L.TstwoError, match="0 has no inverse"):
        L.call("tstwo_check_zero_flag")
    buf.free()


def test_graph_replay_of_every_capturable_op():
    """Eager once (warms the allocator and the scratch), capture the sequence that holds every capturable catalogue op, the three
    GKR scratch users included, then replay three times: new input words copied into the same buffers before each replay (by-value
    scalars are part of the graph and stay), eager calls in between that rewrite scratch, ring, table slot, result page and flag.
    Every replay must give the references' words for ITS inputs."""
    seqs = [SQ.capturable_sequence(d) for d in range(4)]
    assert all(q.signature() == seqs[0].signature() and q.layout() == seqs[0].layout() for q in seqs)
    arena = SQ.Arena(seqs[0])
    staged, h = [], vp()
    try:
        L.sync()
        SQ.enqueue_all(seqs[0], arena.addr)
        msgs = SQ.compare(seqs[0], arena.download())
        assert not msgs, "eager: " + "; ".join(msgs[:6])
        for d in (1, 2, 3):
            b = L.DeviceBuffer(arena.total)
            b.upload(seqs[d].image())
            staged.append(b)
        L.sync()
        L.call("tstwo_graph_begin_capture")
        try:
            SQ.enqueue_all(seqs[0], arena.addr)
        finally:
            L.call("tstwo_graph_end_capture", C.byref(h))
        for step, d in enumerate((1, 2, 3)):
            L.call("tstwo_copy", vp(arena.buf.ptr), vp(staged[step].ptr), arena.total)
            L.call("tstwo_graph_launch", h)
            _eager_state_rewriters(step)
            msgs = SQ.compare(seqs[d], arena.download())
            assert not msgs, f"replay {step}: " + "; ".join(msgs[:6])
        L.call("tstwo_check_zero_flag")                   # the captured inverses met no zero
    finally:
        L.sync()
        if h.value:
            L.call("tstwo_graph_destroy", h)
        for b in staged:
            b.free()
        arena.free()
