"""csrc/hs_switch.h is the one list of the library's environment switches.  A stand-alone program compiled against that header
alone (host compiler, no HIP) is run as child processes under different environments: defaults, parse rules, integer clamps,
latch times and setters.  Pure Python: the list, the sources and the INTEGRATION.md table name the same variables, and nothing
else in csrc/ reads the environment.  Needs no GPU and no built library."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd", "hamspine", "csrc")
HEADER = os.path.join(CSRC, "hs_switch.h")

# argv is a script: get <id> | set <id> <0|1> | setenv <NAME> <text> | unsetenv <NAME>; every get prints one line
PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "hs_switch.h"
#define GET(id, name, rule, d, latch, setter, doc) if (!strcmp(a[i + 1], #id)) { printf("%lld\n", (long long)hs::sw::id()); known = true; }
#define SET_once(id)
#define SET_per_call(id)
#define SET_settable(id) if (!strcmp(a[i + 1], #id)) { hs::sw::set_##id(atoi(a[i + 2])); known = true; }
#define SET(id, name, rule, d, latch, setter, doc) SET_##latch(id)
int main(int n, char** a) {
    for (int i = 1; i < n;) {
        bool known = false;
        if (!strcmp(a[i], "get") && i + 1 < n) {
            HS_SWITCHES(GET)
            if (!strcmp(a[i + 1], "knockout")) { printf("%lld\n", (long long)hs::sw::knockout()); known = true; }
            i += 2;
        } else if (!strcmp(a[i], "set") && i + 2 < n) {
            HS_SWITCHES(SET)
            i += 3;
        } else if (!strcmp(a[i], "setenv") && i + 2 < n) {
            known = setenv(a[i + 1], a[i + 2], 1) == 0;
            i += 3;
        } else if (!strcmp(a[i], "unsetenv") && i + 1 < n) {
            known = unsetenv(a[i + 1]) == 0;
            i += 2;
        }
        if (!known) { fprintf(stderr, "bad script at word %d\n", i); return 2; }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("switches")
    src = d / "switches.cpp"
    src.write_text(PROGRAM)
    out = {}
    for name, flags in (("release", []), ("measure", ["-DHS_MEASURE"])):
        out[name] = str(d / name)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC, *flags, str(src), "-o", out[name]], check=True)
    return out


def _run(exe, script, **env):
    """the values the script's `get`s print, with only the given HAMSPINE_* variables set"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("HAMSPINE_")}
    e.update({"HAMSPINE_" + k: v for k, v in env.items()})
    r = subprocess.run([exe, *script.split()], env=e, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


TEXTS = ("", "0", "1", "00", "2", "off")


def _by_text(exe, switch, var, texts=TEXTS):
    return [_run(exe, f"get {switch}")[0]] + [_run(exe, f"get {switch}", **{var: t})[0] for t in texts]


def test_defaults_and_first_character_parse_rules(programs):
    exe = programs["release"]
    # unset, then TEXTS: "off only if the text starts with 0" ...
    off_if_0 = [1, 1, 0, 1, 0, 1, 1]
    assert _by_text(exe, "p8", "P8") == off_if_0                      # latched at first use
    assert _by_text(exe, "wgrad_nt", "WGRAD_NT") == off_if_0          # settable
    assert _by_text(exe, "ds_compact", "DS_COMPACT") == off_if_0      # read per call
    # ... and "on only if it starts with 1"
    on_if_1 = [0, 0, 0, 1, 0, 0, 0]
    assert _by_text(exe, "persistent", "PERSISTENT") == on_if_1
    assert _by_text(exe, "overlap", "OVERLAP") == on_if_1
    assert _run(exe, "get overlap", OVERLAP="10") == [1] and _run(exe, "get p8", P8="01") == [0]


def test_integer_switches_and_their_clamps(programs):
    exe = programs["release"]
    assert _by_text(exe, "img_lean", "IMG_LEAN", ("0", "15", "16", "2", "", "off", "-1", "13")) == [13, 0, 15, 0, 2, 0, 0, 15, 13]
    assert _by_text(exe, "wgrad_layers", "WGRAD_LAYERS", ("1", "8", "9", "0", "", "-3", "2")) == [2, 1, 8, 2, 2, 2, 2, 2]
    assert _by_text(exe, "split_units", "SPLIT_UNITS", ("0", "-5", "100", "abc", "")) == [512, 512, 512, 100, 512, 512]
    assert _by_text(exe, "split_max", "SPLIT_MAX", ("7", "0", "64", "-1")) == [64, 7, 64, 64, 64]
    assert _by_text(exe, "xblock_bn", "XBLOCK_BN", ("0", "2", "x", "-1")) == [1, 0, 2, 0, -1]


def test_latched_switches_keep_their_first_reading_and_per_call_ones_follow(programs):
    exe = programs["release"]
    assert _run(exe, "get p8 setenv HAMSPINE_P8 0 get p8") == [1, 1]
    assert _run(exe, "get p8 setenv HAMSPINE_P8 1 get p8 unsetenv HAMSPINE_P8 get p8", P8="0") == [0, 0, 0]
    assert _run(exe, "setenv HAMSPINE_P8 0 get p8") == [0]              # latched at first use, not at start-up
    assert _run(exe, "get wgrad_layers setenv HAMSPINE_WGRAD_LAYERS 5 get wgrad_layers") == [2, 2]
    assert _run(exe, "get overlap setenv HAMSPINE_OVERLAP 1 get overlap") == [0, 0]
    assert _run(exe, "get ds_compact setenv HAMSPINE_DS_COMPACT 0 get ds_compact unsetenv HAMSPINE_DS_COMPACT get ds_compact") == [1, 0, 1]
    assert _run(exe, "get img_lean setenv HAMSPINE_IMG_LEAN 2 get img_lean", IMG_LEAN="15") == [15, 2]
    assert _run(exe, "get xblock_bn setenv HAMSPINE_XBLOCK_BN 0 get xblock_bn") == [1, 0]


def test_a_setter_wins_over_the_environment_before_and_after_the_first_read(programs):
    exe = programs["release"]
    assert _run(exe, "set overlap 1 get overlap") == [1]
    assert _run(exe, "set overlap 0 get overlap setenv HAMSPINE_OVERLAP 1 get overlap", OVERLAP="1") == [0, 0]
    assert _run(exe, "get overlap set overlap 0 get overlap set overlap 1 get overlap", OVERLAP="1") == [1, 0, 1]
    assert _run(exe, "get wgrad_nt set wgrad_nt 1 get wgrad_nt", WGRAD_NT="0") == [0, 1]
    assert _run(exe, "set wgrad_nt 0 get wgrad_nt") == [0]
    assert _run(exe, "set bert_wgrad_chunks 0 get bert_wgrad_chunks set bert_wgrad_chunks 7 get bert_wgrad_chunks") == [0, 1]
    assert _run(exe, "get pack_xcd_spread set pack_xcd_spread 0 get pack_xcd_spread") == [1, 0]


def test_the_knock_out_mask_exists_in_measurement_builds_only(programs):
    assert _run(programs["release"], "get knockout") == [0]
    assert _run(programs["release"], "get knockout", KNOCKOUT="5") == [0]
    assert _run(programs["measure"], "get knockout") == [0]
    assert _run(programs["measure"], "get knockout", KNOCKOUT="5") == [5]


def _names(text):
    return set(re.findall(r"\bHAMSPINE_[A-Z0-9_]+\b", text))


def test_the_header_the_sources_and_the_documented_table_name_the_same_switches():
    header = open(HEADER).read()
    rows = re.findall(r'^\s*X\(\s*(\w+),\s*"(HAMSPINE_[A-Z0-9_]+)",\s*(\w+),\s*(-?\d+),\s*(once|per_call|settable),\s*([\w-]+),\s*"[^"]+"\)', header, flags=re.M)
    listed = {r[1] for r in rows}
    assert len(rows) == len(listed) == len({r[0] for r in rows}) >= 32
    assert listed == _names(header)
    assert all((r[4] == "settable") == r[5].startswith("hs_set_") for r in rows)
    sources = [p for pat in ("*.hip", "*.h") for p in glob.glob(os.path.join(CSRC, pat))]
    assert len(sources) > 20
    used = set().union(*(_names(open(p).read()) for p in sources))
    assert used == listed
    assert [os.path.basename(p) for p in sources if "getenv" in open(p).read()] == ["hs_switch.h"]
    # one table row per switch, with the header's default, latch and setter
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = re.findall(r"^\| `(HAMSPINE_[A-Z0-9_]+)` \| ([^|]+) \| ([^|]+) \| ([^|]+) \| ([^|]+) \|$", doc, flags=re.M)
    assert {t[0] for t in table} == listed and len(table) == len(rows)
    by_name = {r[1]: r for r in rows}
    for name, default, latch, setter, meaning in table:
        _, _, _, d, l, s = by_name[name]
        assert default.strip() == d, name
        assert latch.strip() == l.replace("_", " ") + (", measurement builds only" if name == "HAMSPINE_KNOCKOUT" else ""), name
        assert setter.strip().strip("`") == s, name
        assert meaning.strip(), name
