"""The BN_* environment switches (CPU): csrc/switches.h is the one place that lists them and the one place that reads the environment.

A misspelt switch in a test or tool is silently the default path -- the test then "covers" a kernel it never ran.  These tests hold the
table, the sources and the harness together: no getenv outside switches.h, no BN_* string in the sources that is not a row, no row that
nothing reads, no name placed in an environment by tests/, tools/ or bench.py that is neither a row nor on the short list below, and the
accessors give for every kind what the header documents (compiled with the host compiler, the header is host-only)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc")
TABLE = os.path.join(CSRC, "switches.h")
KINDS = {"present", "on_unless_0", "integer", "int64", "real", "text"}

# BN_* names the harness places in an environment that are NOT switches of the library: read by Python only
HARNESS_ONLY = {
    "BN_LIB",                     # rust-birdnet-onnx_amd/__init__.py: the shared library to load (tools/ab_lib.sh)
    "BN_TEST_ROOT",               # tests/test_gpu_group_rccl_branch.py: tells its child process where the repository is
    "BN_BENCH_EXTRAS_INPROCESS",  # bench.py: run the extra legs in the benchmark's own process
}
# ... and compile-time macros of the diagnostic builds (Makefile `stamps`, tools/mb_probe.cpp), never environment variables
COMPILE_TIME = {"BN_GD_STAMPS", "BN_MB_STAMPS"}


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def table_rows():
    """[(kind, name, default text)] of BN_SWITCH_TABLE, in file order."""
    rows = re.findall(r"^\s*X\((\w+),\s*(BN_[A-Z0-9_]+),\s*(.+?),\s*\"", read(TABLE), flags=re.M)
    assert len(rows) > 80 and all(k in KINDS for k, _, _ in rows), rows[:3]
    names = [n for _, n, _ in rows]
    assert len(set(names)) == len(names), "a switch has two rows: " + ", ".join(sorted(n for n in set(names) if names.count(n) > 1))
    return rows


def other_sources():
    return [p for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p) and p != TABLE and p.endswith((".h", ".cpp", ".hip"))]


def test_only_the_table_reads_the_environment():
    offenders = [f"{os.path.basename(p)}:{i + 1}" for p in other_sources() for i, line in enumerate(read(p).splitlines()) if re.search(r"\bgetenv\s*\(", line)]
    assert not offenders, "getenv outside switches.h: " + ", ".join(offenders)
    assert re.search(r"\bgetenv\s*\(", read(TABLE))


def test_every_switch_in_the_sources_is_a_row_and_every_row_is_read():
    rows = {n for _, n, _ in table_rows()}
    literals, used = {}, set()
    for p in other_sources() + [TABLE]:
        text = read(p)
        for n in re.findall(r"\"(BN_[A-Z0-9_]+)\"", text):
            literals.setdefault(n, os.path.basename(p))
        if p != TABLE:
            used |= set(re.findall(r"\bsw::(BN_[A-Z0-9_]+)\b", text))
    stray = {n: f for n, f in literals.items() if n not in rows}
    assert not stray, f"BN_* strings that are no row of switches.h: {stray}"
    assert not used - rows  # (would not compile either)
    assert not rows - used, "rows of switches.h that nothing reads: " + ", ".join(sorted(rows - used))


def names_placed_in_environments():
    """{name: first file}: quoted BN_* names (os.environ keys, monkeypatch.setenv / delenv, env dictionaries, switch sets) and NAME=
    words (keyword arguments of dict(os.environ, ...), assignments of the shell tools) in tests/*.py, tools/* and bench.py."""
    found = {}
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + sorted(glob.glob(os.path.join(ROOT, "tools", "*"))) + [os.path.join(ROOT, "bench.py")]
    for p in files:
        if not os.path.isfile(p) or os.path.abspath(p) == os.path.abspath(__file__):
            continue
        text = read(p)
        for n in re.findall(r"[\"'](BN_[A-Z0-9_]*[A-Z0-9])[\"']", text) + re.findall(r"\b(BN_[A-Z0-9_]*[A-Z0-9])=(?!=)", text):
            found.setdefault(n, os.path.relpath(p, ROOT))
    return found


def test_every_name_the_harness_sets_is_a_switch():
    rows = {n for _, n, _ in table_rows()}
    # constants and enums the C ABI header DEFINES (its comments also name switches)
    abi = set(re.findall(r"^\s*(?:#define\s+)?(BN_[A-Z0-9_]+)\b", read(os.path.join(ROOT, "include", "birdnet_hip.h")), flags=re.M))
    assert {"BN_ABI_VERSION", "BN_ERR_BACKEND", "BN_CTX_NO_GRAPH", "BN_SHARING_SHARED"} <= abi
    assert not (rows & (abi | HARNESS_ONLY | COMPILE_TIME)), "a switch shares its name with something else"
    found = names_placed_in_environments()
    assert len(set(found) & rows) > 50, "the scan no longer sees the switch sets of the GPU tests"
    unknown = {n: f for n, f in found.items() if n not in rows | abi | HARNESS_ONLY | COMPILE_TIME}
    assert not unknown, f"set by the harness, read by nothing (a misspelt switch runs the default path): {unknown}"


PROBE = r"""
#include <cstdio>
#include <cstring>
#include "switches.h"
using namespace bn;
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "table")) {
        for (const SwInfo &r : kSwitchTable) printf("%s %s %s\n", r.kind, r.name, r.dflt);
        return 0;
    }
    printf("present=%d\n", (int)sw_present(sw::BN_NO_GRAPH));
    printf("on=%d\n", (int)sw_on(sw::BN_DWMAP));
    printf("int=%d\n", sw_int(sw::BN_GEMM3));
    printf("int_off=%d\n", (int)(sw_int(sw::BN_STRICT_GRAPH) != 0));
    printf("i64=%lld\n", (long long)sw_i64(sw::BN_MBMAP_MAXHW));
    printf("real=%g\n", sw_double(sw::BN_MBFUSE_HALO));
    printf("text=[%s]\n", sw_text(sw::BN_STFT));
    printf("is_force=%d\n", (int)sw_is(sw::BN_MBFUSE, "force"));
    printf("set=%d\n", (int)sw_is_set(sw::BN_MBROW_TOH));
    return 0;
}
"""
PROBE_VARS = ["BN_NO_GRAPH", "BN_DWMAP", "BN_GEMM3", "BN_STRICT_GRAPH", "BN_MBMAP_MAXHW", "BN_MBFUSE_HALO", "BN_STFT", "BN_MBFUSE", "BN_MBROW_TOH"]
# value of every probed variable (None: unset) -> what each kind reads, as documented at the top of switches.h
EXPECTED = {
    None:    dict(present=0, on=1, int=2, int_off=0, i64=512, real=3, text="auto", is_force=0, set=0),
    "0":     dict(present=1, on=0, int=0, int_off=0, i64=0, real=0, text="0", is_force=0, set=1),
    "1":     dict(present=1, on=1, int=1, int_off=1, i64=1, real=1, text="1", is_force=0, set=1),
    "00":    dict(present=1, on=1, int=0, int_off=0, i64=0, real=0, text="00", is_force=0, set=1),
    "":      dict(present=1, on=1, int=0, int_off=0, i64=0, real=0, text="", is_force=0, set=1),
    "force": dict(present=1, on=1, int=0, int_off=0, i64=0, real=0, text="force", is_force=1, set=1),
}


def host_compile(args):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC] + args, capture_output=True, text=True)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("switches")
    src, out = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    r = host_compile(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(out)])
    if r.returncode != 0 and ("-lasan" in r.stderr or "-lubsan" in r.stderr or "libasan" in r.stderr):
        r = host_compile(["-O1", str(src), "-o", str(out)])  # no sanitizer runtime in this image: the plain build still checks every value
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return str(out), d


def run_probe(binary, args, value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BN_")}
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    if value is not None:
        env.update({k: value for k in PROBE_VARS})
    r = subprocess.run([binary] + args, capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("value", list(EXPECTED), ids=["unset", "0", "1", "00", "empty", "force"])
def test_accessors_read_each_kind_as_documented(probe, value):
    got = dict(line.split("=", 1) for line in run_probe(probe[0], [], value).splitlines())
    want = {k: (f"[{v}]" if k == "text" else str(v)) for k, v in EXPECTED[value].items()}
    assert got == want


def test_compiled_table_is_the_table_in_the_header(probe):
    compiled = [tuple(line.split(" ", 2)) for line in run_probe(probe[0], ["table"], None).splitlines()]
    assert compiled == [(k, n, d.strip()) for k, n, d in table_rows()]


@pytest.mark.parametrize("line,why", [("sw_int(sw::BN_NO_GRAPH)", "wrong kind"), ("sw_present(sw::BN_GEMM3)", "wrong kind"),
                                      ("sw_on(sw::BN_STFT)", "wrong kind"), ("sw_int(sw::BN_NO_SUCH_SWITCH)", "unknown name")])
def test_wrong_kind_or_unknown_name_does_not_compile(probe, line, why):
    src = probe[1] / "bad.cpp"
    good = '#include "switches.h"\nint main() { using namespace bn; return (int)%s; }\n'
    src.write_text(good % "sw_int(sw::BN_GEMM3)")
    assert host_compile(["-fsyntax-only", str(src)]).returncode == 0
    src.write_text(good % line)
    assert host_compile(["-fsyntax-only", str(src)]).returncode != 0, f"{line} ({why}) compiled"
