"""The launch programs the plan builder emits, pinned (CPU, emulated library): tools/plan_signature.py signs every case x switch setting -- launch counts,
cost sums, memory / arena bytes, count and SHA-256 of the DDIF_DUMP_PLAN lines, or the refusal -- and each must equal tests/golden/plan_signature_emu.json field
by field.  The fixture was recorded on the commit BEFORE the builder (csrc/ddif_plan.cpp) was split into stages: a change that restructures the builder keeps
every signature; one that has to change a signature has changed what a plan launches, and says so by re-recording the fixture in a change of its own."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import plan_signature as ps  # noqa: E402
from ddif_testlib import ensure_emu_lib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_signature_emu.json")


def test_fixture_covers_every_case_under_every_setting():
    want = json.load(open(FIXTURE))
    assert sorted(want) == sorted(ps.setting_name(e) for e in ps.SETTINGS)
    for setting, cases in want.items():
        assert sorted(cases) == sorted(ps.case_name(c) for c in ps.CASES), setting


def test_plan_signatures_match_the_recorded_ones(tmp_path):
    want = json.load(open(FIXTURE))
    got, lines = ps.collect(ensure_emu_lib(), "cpu")
    bad = []
    for env in ps.SETTINGS:
        setting = ps.setting_name(env)
        for case in ps.CASES:
            name = ps.case_name(case)
            w, g = want[setting][name], got[setting][name]
            fields = [f for f in sorted(set(w) | set(g)) if w.get(f) != g.get(f)]
            if fields:
                path = tmp_path / ("%s__%s.txt" % (setting.replace(" ", "_").replace("=", ""), name))
                path.write_text("\n".join(lines[setting][name]) + "\n")
                for f in fields:
                    bad.append("[%s] %s: %s = %r, recorded %r  (lines: %s)" % (setting, name, f, g.get(f), w.get(f), path))
    assert not bad, "\n".join(bad)
