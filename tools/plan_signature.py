"""Signature of the launch programs the plan builder (dif-pan_amd/csrc/ddif_plan.cpp) emits: for a fixed list of (data set, B, H, W, inference | train) cases under
a fixed list of environment-switch settings, what a plan reports about itself -- launch counts, cost sums, memory (the arena size depends on the order of the
builder's allocations) -- and a SHA-256 of the `[ddif plan]` lines DDIF_DUMP_PLAN=1 writes while the plan is created (every conv of both programs: layer, kernel
instantiation, cfg, prologue / epilogue bits, items, grid, LDS bytes; the two trailing pointer fields are removed, nothing else is normalised).  A refused plan
signs with its error code and message.  A change that only restructures the builder leaves every field as it is (tests/test_plan_signature.py compares against
tests/golden/plan_signature_emu.json, recorded on the emulated library).

The library reads its switches once per process: every setting runs all cases in ONE child process started with that environment.

usage: plan_signature.py --lib PATH --device cpu|cuda [--dump CASE [--setting NAME]]
  prints one JSON object {setting: {case: signature}}; --dump prints the normalised lines of one case instead (to diff two trees by hand)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (data set, B, H, W, train)
CASES = [
    ("wv3", 1, 64, 64, False),  # the 132-launch program: linattn_fused, linattn8_fused, attn_block, EPI_XF
    ("wv3", 2, 16, 16, False),
    ("gf2", 2, 32, 32, False),
    ("cave", 1, 32, 32, False),  # 31-channel stem (scalar staging), Cout % 4 != 0
    ("wv3", 1, 24, 40, False),  # non-square, partial tiles
    ("wv3", 2, 16, 16, True),
    ("wv3", 1, 64, 64, True),
]

SETTINGS = [
    {},
    {"DDIF_LAFUSE": "0"},
    {"DDIF_LA8": "0", "DDIF_LA6": "0"},
    {"DDIF_XF": "0"},
    {"DDIF_LR": "0"},
    {"DDIF_X3": "0", "DDIF_F16": "0"},  # the exact_fp32 bracket of bench.py
    {"DDIF_TILE16": "0", "DDIF_WRES": "0", "DDIF_XCD": "0"},
    {"DDIF_S2_F16": "0", "DDIF_ATTN_F16": "0", "DDIF_LR_ROWS": "0", "DDIF_LA_NW": "4"},
    {"DDIF_MATH": "bf16"},
    {"DDIF_TRAIN_X3": "0"},
]


def case_name(case) -> str:
    ds, B, H, W, train = case
    return "%s_b%d_%dx%d_%s" % (ds, B, H, W, "train" if train else "infer")


def setting_name(env) -> str:
    return " ".join("%s=%s" % kv for kv in env.items()) or "default"


_PTRS = re.compile(r"\s+in@\S+\s+out@\S+\s*$")


def normalise(text: str):
    """The `[ddif plan]` lines of a captured stderr, without their two trailing pointer fields."""
    return [_PTRS.sub("", ln) for ln in text.splitlines() if ln.startswith("[ddif plan]")]


class _CaptureStderr:
    """File-descriptor level: the library writes with fprintf(stderr)."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def _child(lib_path: str, device: str):
    """All cases under THIS process's environment; prints {case: {"sig": ..., "lines": [...]}}."""
    sys.path[:0] = [os.path.join(ROOT, "dif-pan_amd"), ROOT, os.path.join(ROOT, "tests")]
    import torch
    from ddif import runtime
    from ddif_testlib import make_net

    with _CaptureStderr():  # (the emulated build announces itself on stderr)
        lib = runtime.use_library(os.path.abspath(lib_path))
    assert lib.emulated == (device == "cpu"), "--device cpu goes with the emulated library, --device cuda with the gfx950 one"
    dev = torch.device("cuda:0" if device == "cuda" else "cpu")
    dll = lib.dll
    nets, out = {}, {}
    for case in CASES:
        ds, B, H, W, train = case
        if ds not in nets:
            nets[ds] = make_net(ds, dev)
        nh = nets[ds]._ensure_net(dev)
        h = C.c_void_p()
        create = dll.ddif_plan_create_train if train else dll.ddif_plan_create
        with _CaptureStderr() as cap:
            rc = create(C.byref(h), nh.h, B, H, W)
        lines = normalise(cap.text)
        sig = {"dump_lines": len(lines), "dump_sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}
        if rc != 0:
            sig["error"] = [int(rc), dll.ddif_last_error().decode(errors="replace")]
        else:
            a, b = C.c_int(), C.c_int()
            lib.check(dll.ddif_plan_num_launches(h, C.byref(a), C.byref(b)), "ddif_plan_num_launches")
            sig["num_launches"] = [a.value, b.value]
            d = [C.c_double() for _ in range(4)]
            lib.check(dll.ddif_plan_cost(h, *[C.byref(x) for x in d]), "ddif_plan_cost")
            sig["cost"] = [x.value.hex() for x in d]  # exact: sums of the same terms in the same order
            m = [C.c_int64() for _ in range(3)]
            lib.check(dll.ddif_plan_memory(h, *[C.byref(x) for x in m]), "ddif_plan_memory")
            sig["memory"] = [x.value for x in m]
            dll.ddif_plan_destroy(h)
        out[case_name(case)] = {"sig": sig, "lines": lines}
    sys.stdout.write(json.dumps(out) + "\n")


def run_setting(lib_path: str, device: str, env: dict):
    """One child process for one switch setting -> ({case: signature}, {case: normalised lines})."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("DDIF_")}
    e.update(env)
    e["DDIF_DUMP_PLAN"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib_path, "--device", device, "--child"], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("plan_signature child failed under [%s] (exit %d):\n%s" % (setting_name(env), r.returncode, (r.stdout + r.stderr)[-3000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: v["sig"] for k, v in res.items()}, {k: v["lines"] for k, v in res.items()}


def collect(lib_path: str, device: str):
    """({setting: {case: signature}}, {setting: {case: normalised lines}}) over SETTINGS x CASES."""
    from concurrent.futures import ThreadPoolExecutor

    # (the emulator builds plans on the host: several children side by side; the GPU children take turns)
    with ThreadPoolExecutor(max_workers=5 if device == "cpu" else 1) as pool:
        res = list(pool.map(lambda env: run_setting(lib_path, device, env), SETTINGS))
    names = [setting_name(env) for env in SETTINGS]
    return {n: r[0] for n, r in zip(names, res)}, {n: r[1] for n, r in zip(names, res)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True)
    ap.add_argument("--device", required=True, choices=["cpu", "cuda"])
    ap.add_argument("--dump", metavar="CASE", help="print the normalised lines of one case (names: %s)" % ", ".join(case_name(c) for c in CASES))
    ap.add_argument("--setting", default="default", help="with --dump: the switch setting, as the JSON output names it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return _child(a.lib, a.device)
    if a.dump:
        env = next((s for s in SETTINGS if setting_name(s) == a.setting), None)
        if env is None or a.dump not in [case_name(c) for c in CASES]:
            ap.error("unknown case or setting")
        print("\n".join(run_setting(a.lib, a.device, env)[1][a.dump]))
        return
    print(json.dumps(collect(a.lib, a.device)[0], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
