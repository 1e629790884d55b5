"""CPU-only: the two planning knobs of libkmx's host code (kmtricks_amd/csrc/kmx_host.hpp).  kmx_plan_cus and
kmx_grid_cap compiled into a small host program and asked what they return for a list of environments -- unset and anything out of
range give the device's CU count and the built-in cap --, and the sources read for where the helpers are used: the launches the
section lists, and nothing of the merge, count and super-k-mer paths."""
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmtricks_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROBE = r"""
#include "kmx_host.hpp"
#include <cstdio>
int main(int argc, char** argv) {
  kmx_ctx* c = new kmx_ctx();      // (never destroyed: no device call is made)
  c->n_cu = atoi(argv[1]);
  printf("%d %u %u\n", kmx_plan_cus(c), kmx_grid_cap(1u << 18), kmx_grid_cap(1u << 20));
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O0", f"-I{CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def ask(n_cu, **env):
        e = {k: v for k, v in os.environ.items() if k not in ("KMX_PLAN_CUS", "KMX_MAX_GRID")}
        e.update(env)
        out = subprocess.run([str(exe), str(n_cu)], capture_output=True, text=True, env=e)
        assert out.returncode == 0, out.stderr
        return tuple(int(x) for x in out.stdout.split())
    return ask


def test_unset_gives_the_device_and_the_built_in_caps(probe):
    assert probe(256) == (256, 1 << 18, 1 << 20)
    assert probe(1) == (1, 1 << 18, 1 << 20)


def test_plan_cus_only_lowers_the_count(probe):
    for text, want in (("1", 1), ("8", 8), ("255", 255), ("256", 256), ("257", 256), ("0", 256), ("-1", 256), ("", 256), ("x", 256), ("8x", 256),
                       (" 8", 256), ("+8", 256), ("0x10", 256), ("1e2", 256), ("99999999999999999999", 256), ("4294967297", 256)):
        assert probe(256, KMX_PLAN_CUS=text)[0] == want, text
        assert probe(256, KMX_PLAN_CUS=text)[1:] == (1 << 18, 1 << 20), text      # (the other knob is untouched)
    assert probe(4, KMX_PLAN_CUS="8")[0] == 4


def test_grid_cap_only_lowers_the_cap(probe):
    for text, want in (("1", (1, 1)), ("3", (3, 3)), ("262144", (1 << 18, 1 << 18)), ("262145", (1 << 18, 262145)), ("1048576", (1 << 18, 1 << 20)),
                       ("1048577", (1 << 18, 1 << 20)), ("0", (1 << 18, 1 << 20)), ("-3", (1 << 18, 1 << 20)), ("", (1 << 18, 1 << 20)),
                       ("three", (1 << 18, 1 << 20)), ("3 ", (1 << 18, 1 << 20)), ("4294967299", (1 << 18, 1 << 20))):
        assert probe(256, KMX_MAX_GRID=text) == (256,) + want, text


def uses(name, word):
    return len(re.findall(r"\b%s\b" % word, open(os.path.join(CSRC, name)).read()))


def test_the_helpers_are_used_where_the_design_says_and_nowhere_else():
    plan = {"diff.hip": 2, "select.hip": 1, "dist.hip": 1, "query.hip": 1, "kquery.hip": 3, "cquery.hip": 1, "zquery.hip": 2}
    cap = {"filter.hip": 1, "combine.hip": 1, "diff.hip": 2, "select.hip": 3, "dist.hip": 1}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp", ".h")) or name == "kmx_host.hpp":
            continue
        assert uses(name, "kmx_plan_cus") == plan.get(name, 0), name
        assert uses(name, "kmx_grid_cap") == cap.get(name, 0), name
        assert not uses(name, "KMX_PLAN_CUS") and not uses(name, "KMX_MAX_GRID"), name      # (read in kmx_host.hpp alone)
    # the one CU count of dist.hip feeds both dist_runs calls
    src = open(os.path.join(CSRC, "dist.hip")).read()
    assert len(re.findall(r"dist_runs\([^;]*\bn_cu\b", src)) == 3 and "n_cu = (u32)std::max(kmx_plan_cus(ctx), 1)" in src
    # what the knobs must not reach: these size scratch and look-back chains by the real CU count
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".hpp", ".h")) and (name == "kmx_api.hip" or name.startswith(("merge_", "count", "superk"))):
            assert not uses(name, "kmx_plan_cus") and not uses(name, "kmx_grid_cap"), name
