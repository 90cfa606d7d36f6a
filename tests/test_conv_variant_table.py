"""The conv variant table, pinned: what get_conv_variant / get_xf_variant (csrc/ddif_plan.h) return for every key of the enumeration below -- whether a kernel
exists and, if so, smem, th, tw, nt, nthr, x3, f16, b1, wg_cap, lr, wr, nbs and the name -- must equal tests/golden/conv_variant_table.json entry by entry, and
no key outside the fixture may have a kernel.  Plans on test-sized shapes never pick some tilings (3 / 4 / 13-16 / 52-56 / 47-49, 67 under the default rule), so
tests/test_plan_signature.py cannot see their LDS sizes; a too small one does not fault on this hardware, it corrupts.

The fixture was recorded on the commit BEFORE the table's rows were derived from the kernel's geometry (ConvGeom, csrc/kernels_conv.h) -- d0b0350, where every
row spelled its launch parameters out by hand -- as tests/golden/plan_signature_emu.json was for the plan builder: only the entry point
(ddif_conv_variant_table, include/ddif_testops.h) and this enumeration were applied to a checkout of that commit, the emulated library built, and
`python tests/test_conv_variant_table.py record` run.  A change that restructures the table keeps every entry; one that adds or changes a tiling re-records.

The lookups launch nothing: the CPU leg reads the emulated library, the gpu leg the gfx950 library, against the same fixture."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_variant_table.json")

# EPI_* bits of csrc/kernels_conv.h
FILM, SOUT, RES, SILU, TBS, COLST, SAMP, XF1, XF2, PRED = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
# every epilogue value the instantiating translation units mention (ddif_conv_k1 / _k3 / _k3e / ddif_xf.cpp; COLST: the low-resolution kernel behind cfg 20 / 21) ...
EPI_MENTIONED = [0, FILM, SOUT, RES, SILU, TBS, COLST, SAMP, SAMP | PRED, XF1, RES | XF1, XF2, RES | XF2]
# ... each with the per-sample time-bias bit (add_conv asks for `epi | EPI_TBS` twins), and one combination no unit has
EPI_VALUES = sorted(set(EPI_MENTIONED) | {e | TBS for e in EPI_MENTIONED} | {FILM | SILU})


VARIANT_FIELDS = ("smem", "th", "tw", "nt", "nthr", "x3", "f16", "b1", "wg_cap", "lr", "wr", "nbs", "name")


class ConvVariantInfo(C.Structure):
    """ddif_conv_variant_info (include/ddif_testops.h)"""
    _fields_ = [("found", C.c_int)] + [(f, C.c_int) for f in ("th", "tw", "nt", "nthr", "x3", "f16", "b1", "wg_cap", "lr", "wr", "nbs")] + [
        ("smem", C.c_int64), ("name", C.c_char_p)]


def conv_variant_table(keys, xf=False):
    """ddif_conv_variant_table of the library the binding has loaded: {key: [VARIANT_FIELDS values]} for the keys that have a kernel.  keys: tuples of
    get_conv_variant's nine arguments, or with xf of get_xf_variant's six.  (Bound here, not in tests/ddif_testops.py: that module is shared by the whole suite.)"""
    from ddif import runtime

    lib = runtime.get_lib()
    lib.dll.ddif_conv_variant_table.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(ConvVariantInfo)]
    k = np.asarray(keys, dtype=np.int32)
    n, w = k.shape
    flat = np.zeros((n, 9), dtype=np.int32)
    flat[:, :w] = k
    out = (ConvVariantInfo * n)()
    lib.check(lib.dll.ddif_conv_variant_table(1 if xf else 0, flat.ctypes.data_as(C.POINTER(C.c_int)), n, out), "ddif_conv_variant_table")
    found = np.frombuffer(out, dtype=np.int32).reshape(n, C.sizeof(ConvVariantInfo) // 4)[:, 0]  # (most keys have no kernel: look at those that do only)
    return {tuple(int(v) for v in k[i]): [out[i].name.decode() if f == "name" else int(getattr(out[i], f)) for f in VARIANT_FIELDS] for i in np.nonzero(found)[0]}


def conv_keys():
    """(ks, stride, ups, ck, pro, cfg, vec, epi, math) in chunks of one (ks, stride, ups, ck)"""
    for head in itertools.product((1, 3), (1, 2), (0, 1), (16, 32)):
        yield [head + tail for tail in itertools.product(range(5), range(70), range(3), EPI_VALUES, range(3))]


def xf_keys():
    """(stride, pro, cfg, vec, epi, nbx): the x_conv-fold domain"""
    return list(itertools.product((1, 2), range(5), (27, 28, 37, 67, 68), range(3), (0, RES), (1, 2)))


def collect():
    conv = {}
    for chunk in conv_keys():
        conv.update(conv_variant_table(chunk))
    return {"conv": conv, "xf": conv_variant_table(xf_keys(), xf=True)}


def as_rows(table):
    return [list(k) + v for k, v in sorted(table.items())]


def check_against_fixture():
    want = json.load(open(FIXTURE))
    got = collect()
    bad = []
    for part, nkey in (("conv", 9), ("xf", 6)):
        w = {tuple(r[:nkey]): r[nkey:] for r in want[part]}
        g = got[part]
        assert len(w) == len(want[part]), "duplicate keys in the fixture"
        for k in sorted(set(w) | set(g)):
            if w.get(k) != g.get(k):
                bad.append("%s %s: %s, recorded %s" % (part, k, g.get(k), w.get(k)))
    assert not bad, "%d entries differ (fields: %s)\n%s" % (len(bad), ", ".join(want["fields"]), "\n".join(bad[:40]))


def test_fixture_sees_the_tilings_plans_never_pick():
    want = json.load(open(FIXTURE))
    assert want["fields"] == list(VARIANT_FIELDS)
    cfgs = {r[5] for r in want["conv"]}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 20, 21, 27, 28, 29, 37, 47, 48, 49, 52, 53, 54, 55, 56, 67, 68} == cfgs
    assert {r[2] for r in want["xf"]} == {27, 28, 37, 68}


def test_variant_table_matches_the_recorded_one_emulated():
    from ddif_testlib import use_emulator

    assert use_emulator().emulated
    check_against_fixture()


@pytest.mark.gpu
def test_variant_table_matches_the_recorded_one_gfx950():
    from ddif_testlib import use_gpu_library

    use_gpu_library()
    check_against_fixture()


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    sys.path[:0] = [os.path.join(ROOT, "dif-pan_amd"), os.path.join(ROOT, "tests"), ROOT]
    from ddif_testlib import use_emulator

    assert use_emulator().emulated
    got = collect()
    with open(FIXTURE, "w") as f:
        f.write('{"fields": %s,\n "conv": [\n  %s\n ],\n "xf": [\n  %s\n ]}\n' % (json.dumps(list(VARIANT_FIELDS)), ",\n  ".join(json.dumps(r) for r in as_rows(got["conv"])),
                                                                         ",\n  ".join(json.dumps(r) for r in as_rows(got["xf"]))))
    print("recorded %d conv and %d xf entries" % (len(got["conv"]), len(got["xf"])))
