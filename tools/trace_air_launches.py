#!/usr/bin/env python3
"""Every AIR entry at every shape of tests/air_plan.py gpu_shapes(), to compare two builds of the library (TSTWO_HIP_LIB selects
one) launch by launch, and the host cost of the two entries a prover calls most.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trace_air_launches.py     (a run of its own: no counters)
    python tools/trace_air_launches.py --list DIR > launches.txt     one line per launch, in start order: name, grid, workgroup, LDS
    python tools/trace_air_launches.py --diff A.txt B.txt            exit 1 unless the lists agree line by line
    python tools/trace_air_launches.py --host-cost [--reps 1000]     us per call of tstwo_air_eval_program and
                                                                      tstwo_air_eval_columns_compiled at log 8, enqueue to return

The programs are tests/air_plan.py register_program: as many registers as the shape names (the LDS of a launch), one terminal per
constraint or output.  Columns of one call share one buffer of zeros, outputs and accumulators are their own: only the launches
matter here."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STORE = 8


def launches(root):
    import csv, glob
    rows = []
    for f in glob.glob(f"{root}/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{name} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}x{r['Grid_Size_Z']} wg {r['Workgroup_Size_X']}x{r['Workgroup_Size_Y']}x{r['Workgroup_Size_Z']}"
              f" lds {r.get('LDS_Block_Size', '?')}")


def diff(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad = abs(len(la) - len(lb))
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            bad += 1
            print(f"line {i + 1}: {x}  |  {y}")
    print(f"{len(la)} / {len(lb)} launches, {bad} differ")
    return 1 if bad else 0


class Caller:
    """One call per shape; kernels compiled once per (kind, columns, terminals)."""

    def __init__(self):
        import re
        from tstwo_amd import _lib as L
        from tstwo_amd.backend import HipColumn
        import air_plan
        self.L, self.HipColumn, self.AP = L, HipColumn, air_plan
        L.init(0)
        self.n_cus = int(re.search(r"(\d+) CUs", L.device_name()).group(1))
        self.kernels = {}
        self.bufs = {}

    def buf(self, name, log):
        """A device buffer of 2^log + 4 zero words, kept by name and size."""
        if (name, log) not in self.bufs:
            self.bufs[name, log] = self.HipColumn.zeros((1 << log) + 4)
        return self.bufs[name, log]

    def kernel(self, entry, words, n_cols, n_terminal):
        key = (entry, tuple(words), n_cols, n_terminal)
        if key not in self.kernels:
            kid = C.c_uint64(0)
            self.L.call("tstwo_air_program_compile" if entry == "eval_compiled" else "tstwo_air_columns_compile", self.L.u32x(words), len(words) // 2,
                        n_cols, n_terminal, C.byref(kid))
            self.kernels[key] = kid.value
        return self.kernels[key]

    def call(self, i):
        self.L.call(*self.prepare(i))

    def prepare(self, i):
        """The arguments of L.call for the shape."""
        L, AP = self.L, self.AP
        off = 0 if i.aligned else 4
        cols = L.ptr_array([self.buf("in", i.log).ptr + off] * i.n_cols)
        acc = L.p4([self.buf(f"acc{j}", i.log).ptr + off for j in range(4)])
        coeffs, dinv = L.u32x([1, 0, 0, 0] * max(i.n_terminal, 1)), L.u32x([1] * (1 << i.log_expand))
        trace_log = i.log - i.log_expand
        n_regs = i.n_regs or 2
        if i.entry == "wide_fib_trace":
            out = L.ptr_array([self.buf("out0", i.log).ptr + off] * i.n_cols)
            return ("tstwo_air_wide_fib_trace", C.c_void_p(self.buf("in", i.log).ptr + off), C.c_void_p(self.buf("in", i.log).ptr + off), i.log, out, i.n_cols)
        if i.entry == "quotients":
            return ("tstwo_air_constraint_quotients", i.kind, cols, i.n_cols, trace_log, i.log_expand, coeffs, i.n_terminal, dinv, acc)
        if i.entry in ("eval_program", "eval_compiled"):
            words = AP.register_program(n_regs, i.n_cols, [0] * i.n_terminal)
            if i.entry == "eval_program":
                return ("tstwo_air_eval_program", cols, i.n_cols, trace_log, i.log_expand, L.u32x(words), len(words) // 2, coeffs, i.n_terminal, dinv, acc)
            return ("tstwo_air_eval_compiled", self.kernel(i.entry, words, i.n_cols, i.n_terminal), cols, i.n_cols, trace_log, i.log_expand, coeffs,
                    i.n_terminal, dinv, acc)
        if i.entry in ("eval_columns", "eval_columns_compiled"):
            words = AP.register_program(n_regs, i.n_cols, list(range(i.n_terminal)), STORE)
            out = L.ptr_array([self.buf(f"out{k}", i.log).ptr + off for k in range(i.n_terminal)])
            if i.entry == "eval_columns":
                return ("tstwo_air_eval_columns", cols, i.n_cols, i.log, L.u32x(words), len(words) // 2, out, i.n_terminal)
            return ("tstwo_air_eval_columns_compiled", self.kernel(i.entry, words, i.n_cols, i.n_terminal), cols, i.n_cols, i.log, out, i.n_terminal)
        words = AP.register_program(n_regs, i.n_cols, list(range(i.n_terminal)))
        return ("tstwo_air_check_constraints", cols, i.n_cols, i.log, L.u32x(words), len(words) // 2, i.n_terminal, C.c_void_p(self.buf("report", 9).ptr))


def run():
    c = Caller()
    shapes = c.AP.gpu_shapes(c.n_cus)
    for name, i in shapes.items():
        c.call(i)
        if i.log >= 20:
            c.L.sync()
            c.bufs = {k: v for k, v in c.bufs.items() if k[1] < 20}          # the large buffers, one size at a time
    c.L.sync()
    print(f"done: {len(shapes)} shapes on {c.n_cus} CUs", flush=True)


def host_cost(reps):
    c = Caller()
    AP = c.AP
    shapes = {"tstwo_air_eval_program": AP.Input("eval_program", 0, 8, 1, 3, 2, 0, 4, True, c.n_cus),
              "tstwo_air_eval_columns_compiled": AP.Input("eval_columns_compiled", 0, 8, 0, 3, 2, 0, 0, True, c.n_cus)}
    for name, i in shapes.items():
        args = c.prepare(i)
        for _ in range(50):
            c.L.call(*args)
        c.L.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.L.call(*args)
            ts.append(time.perf_counter() - t0)
            if len(ts) % 100 == 0:
                c.L.sync()
        c.L.sync()
        ts.sort()
        print(f"{name} log 8, {reps} calls: avg {1e6 * sum(ts) / len(ts):.2f} us  median {1e6 * ts[len(ts) // 2]:.2f} us  min {1e6 * ts[0]:.2f} us", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--list":
        launches(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--host-cost":
        host_cost(int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[2] == "--reps" else 1000)
    else:
        run()
