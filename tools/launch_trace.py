#!/usr/bin/env python
"""What tools/isa_diff.py is for kernel refactors, for host refactors: every launch of one seeded training step per case, one line
each -- the entry point and its arguments, pointers as the ordinal of their first appearance in the case (`null` for NULL; with
--no-ordinals just `ptr`), every field of every problem of a grouped GEMM.  Two trees make the same launches when their outputs
are identical under diff.  Needs a GPU.
    python tools/launch_trace.py [--pkg DIR_HOLDING_ANOTHER_kbner] [--no-ordinals] > trace.txt"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = sys.argv[sys.argv.index("--pkg") + 1] if "--pkg" in sys.argv else os.path.join(ROOT, "kb-ner_amd")
sys.path[:0] = [os.path.abspath(PKG), ROOT, os.path.join(ROOT, "tests")]

from kbner import lib as L  # noqa: E402
import test_gpu_head_rows_e2e as t  # noqa: E402  (its three configurations, batch and seeded step)

seen = {}


def fmt(x):
    if isinstance(x, ctypes.Array):     # host records of a batched reduction: device addresses and small counts
        return "[%s]" % " ".join(fmt(ctypes.c_void_p(v)) if v >> 32 else str(v) for v in x)
    if x is None or isinstance(x, ctypes.c_void_p):
        v = getattr(x, "value", None)
        return "null" if not v else "p%d" % seen.setdefault(v, len(seen)) if "--no-ordinals" not in sys.argv else "ptr"
    return "%.9g" % x if isinstance(x, float) else str(x)


def call(name, *args):
    grouped = name.startswith("kbner_gemm_bf16_grouped")     # (its third argument is the host array of problems, printed below)
    print(name, *(fmt(x) for i, x in enumerate(args) if not (grouped and i == 2)))
    if grouped:
        for q in (L.GemmProblem * args[1]).from_address(args[2].value):
            print("   ", *("%s=%s" % (f, fmt(ctypes.c_void_p(getattr(q, f)) if ty is L.P else getattr(q, f))) for f, ty in q._fields_))
    return real_call(name, *args)


real_call, L.call = L.call, call
print("tracing", os.path.dirname(L.__file__), file=sys.stderr)
for name, c in t.CONFIGS.items():
    bd = t.kb.to_device(t.uneven_batch(c["B"], c["S"], c["V"]), t.DEV)
    for rows, dropout, defer in [(r, d, None) for r in (True, False) for d in (False, True)] + [(True, True, 0)] * (name == "routes"):
        seen.clear()
        print("== %s head_rows_only=%s dropout=%s defer_max=%s" % (name, rows, dropout, defer))
        tg = t.make_tagger(c, rows)[1]
        if defer is not None:
            tg.DEFER_REDUCE_MAX_TOKENS = defer
        t.run_step(tg, bd, dropout, 0.0)
    if name == "small":
        seen.clear()
        print("== small forward_features, no graph")
        tg = t.make_tagger(c, True)[1]
        tg.INFER_GRAPH = False
        tg.forward_features(bd)
