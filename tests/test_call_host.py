"""The launch paths' call contract without a GPU: csrc/tt_call_host.h (range checks, flag decode, device-count
refusals, alignment) run by a stand-alone program under ASan + UBSan over a table of rows. Each row carries
the status, tt_last_error text and plan the C ABI promises (a host may match on the texts); rows that break two
conditions at once pin the order of the checks."""
import os
import subprocess

import tthip

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

OK, BAD = tthip.TT_OK, tthip.TT_ERR_INVALID_ARG
DEV, STATS, ASYNC = tthip.TT_TRACE_DEVICE_PTRS, tthip.TT_TRACE_STATS, tthip.TT_TRACE_ASYNC
ALIGNED, OFF4 = 0x7F0000001000, 0x7F0000001004  # pointer values (never dereferenced)

T_NULL, T_NULL_SH = "null params or rays", "null params or shadow rays"
T_SCREEN0, T_BOUNCE, T_LARGE, T_RANGE = "zero screen size", "negative bounce", "screen too large", "ray range overflows"
T_CNT_DEV = "a device-resident ray count needs TT_TRACE_DEVICE_PTRS"
T_CNT_STATS = "TT_TRACE_STATS needs a host ray count"
T_CNT_MEM = "the ray count pointer is not device memory"
T_ALIGN = "GlobalRays / _PrimaryTriangleInfo must be 16-byte aligned"
T_ALIGN_SH = "shadow rays / visibility / NEEPosA must be 16-byte aligned"
T_ENQ_NULL, T_ENQ_BAD = "null argument", "bad ray count / screen"
T_ENQ_DEV = "device-resident ray counts need TT_TRACE_DEVICE_PTRS"


def row(name, path, want, text="", plan=None, *, args=True, n=64, w=8, h=8, bounce=0, flags=0, count=False,
        count_dev=True, a=ALIGNED, b=0, c=0):
    """plan: (wh, off, dst, dev, async, stats) of an accepted call"""
    assert (want == OK) == (plan is not None) and "\t" not in text
    p = "-" if plan is None else " ".join(str(int(v)) for v in plan)
    cells = [name, path, int(args), n, w, h, bounce, flags, int(count), int(count_dev), a, b, c, want, text, p]
    return "\t".join(str(v) for v in cells)


def table():
    R = []
    # the 2^31 and 2^32 limits
    R.append(row("wh 2^31-1", "trace", OK, plan=(0x7FFFFFFF, 0, 0, 0, 0, 0), w=0x7FFFFFFF, h=1))
    R.append(row("wh 2^31", "trace", BAD, T_LARGE, w=0x80000000, h=1))
    R.append(row("wh 2^31 as 65536 x 32768", "shadow", BAD, T_LARGE, w=65536, h=32768))
    R.append(row("off + n = 2^32-1", "trace", OK, plan=(0x7FFFFFFF, 0x7FFFFFFF, 0, 0, 0, 0), w=0x7FFFFFFF, h=1, bounce=1,
                 n=0x80000000))
    R.append(row("off + n = 2^32", "trace", BAD, T_RANGE, w=0x7FFFFFFF, h=1, bounce=1, n=0x80000001))
    R.append(row("off + n = 2^32, heightmap", "heightmap", BAD, T_RANGE, w=0x7FFFFFFF, h=1, bounce=3, n=0x80000001))
    R.append(row("no ray window on the shadow path", "shadow", OK, plan=(0x7FFFFFFF, 0, 0, 0, 0, 0), w=0x7FFFFFFF, h=1,
                 bounce=1, n=0xFFFFFFFF))
    # even and odd bounce
    R.append(row("bounce 0", "trace", OK, plan=(64, 0, 0, 0, 0, 0), bounce=0))
    R.append(row("bounce 1", "trace", OK, plan=(64, 64, 0, 0, 0, 0), bounce=1))
    R.append(row("bounce 2", "heightmap", OK, plan=(64, 0, 0, 0, 0, 0), bounce=2))
    R.append(row("bounce 5", "heightmap", OK, plan=(64, 64, 0, 0, 0, 0), bounce=5))
    # dev / async
    R.append(row("host pointers", "trace", OK, plan=(64, 0, 0, 0, 0, 0)))
    R.append(row("ASYNC without DEVICE_PTRS is synchronous", "trace", OK, plan=(64, 0, 0, 0, 0, 0), flags=ASYNC))
    R.append(row("DEVICE_PTRS alone is synchronous", "trace", OK, plan=(64, 0, 0, 1, 0, 0), flags=DEV))
    R.append(row("DEVICE_PTRS | ASYNC", "shadow", OK, plan=(64, 0, 0, 1, 1, 0), flags=DEV | ASYNC))
    R.append(row("a device count implies async", "trace", OK, plan=(64, 0, 0, 1, 1, 0), flags=DEV, count=True))
    R.append(row("stats decoded", "shadow", OK, plan=(64, 0, 0, 0, 0, 1), flags=STATS))
    # the three device-count refusals
    R.append(row("count without DEVICE_PTRS", "trace", BAD, T_CNT_DEV, count=True))
    R.append(row("count with stats", "shadow", BAD, T_CNT_STATS, flags=DEV | STATS, count=True))
    R.append(row("count not device memory", "heightmap", BAD, T_CNT_MEM, flags=DEV, count=True, count_dev=False))
    R.append(row("shadow heightmap has no stats form", "shadow_heightmap", OK, plan=(64, 0, 0, 1, 1, 1),
                 flags=DEV | STATS, count=True))
    R.append(row("shadow heightmap: count not device memory", "shadow_heightmap", BAD, T_CNT_MEM, flags=DEV, count=True,
                 count_dev=False))
    # alignment, after the n_rays == 0 return
    R.append(row("misaligned, n_rays 0", "trace", OK, plan=(64, 0, 0, 0, 0, 0), n=0, a=OFF4))
    R.append(row("misaligned, n_rays 1", "trace", BAD, T_ALIGN, n=1, a=OFF4))
    R.append(row("misaligned info", "heightmap", BAD, T_ALIGN, b=OFF4))
    R.append(row("misaligned visibility", "shadow", BAD, T_ALIGN_SH, b=OFF4))
    R.append(row("misaligned NEEPosA", "shadow_heightmap", BAD, T_ALIGN_SH, c=ALIGNED + 8))
    R.append(row("absent arrays are not misaligned", "shadow", OK, plan=(64, 0, 0, 0, 0, 0), b=0, c=0))
    # per-path wording
    R.append(row("null, trace", "trace", BAD, T_NULL, args=False))
    R.append(row("null, shadow", "shadow", BAD, T_NULL_SH, args=False))
    R.append(row("null, shadow heightmap", "shadow_heightmap", BAD, T_NULL_SH, args=False))
    R.append(row("zero width", "shadow", BAD, T_SCREEN0, w=0))
    R.append(row("zero height", "heightmap", BAD, T_SCREEN0, h=0))
    # two conditions at once: the order of the checks
    R.append(row("null rays + zero screen", "trace", BAD, T_NULL, args=False, w=0, h=0))
    R.append(row("negative bounce + screen too large", "trace", BAD, T_BOUNCE, bounce=-1, w=0x80000000, h=1))
    R.append(row("stats + count without DEVICE_PTRS", "trace", BAD, T_CNT_DEV, flags=STATS, count=True))
    R.append(row("zero screen + negative bounce", "shadow", BAD, T_SCREEN0, w=0, bounce=-2))
    R.append(row("screen too large + count without DEVICE_PTRS", "heightmap", BAD, T_LARGE, w=65536, h=65536, count=True))
    R.append(row("range overflow + misaligned", "trace", BAD, T_RANGE, w=0x7FFFFFFF, h=1, bounce=1, n=0x80000001, a=OFF4))
    R.append(row("count not device memory + misaligned", "trace", BAD, T_CNT_MEM, flags=DEV, count=True, count_dev=False,
                 a=OFF4))
    # the bounce enqueue's own contract
    R.append(row("enqueue even", "enqueue", OK, plan=(64, 0, 64, 0, 0, 0), bounce=0))
    R.append(row("enqueue odd", "enqueue", OK, plan=(64, 64, 0, 1, 0, 0), bounce=1, flags=DEV))
    R.append(row("enqueue null", "enqueue", BAD, T_ENQ_NULL, args=False))
    R.append(row("enqueue zero screen", "enqueue", BAD, T_ENQ_BAD, w=0))
    R.append(row("enqueue more rays than pixels", "enqueue", BAD, T_ENQ_BAD, n=65))
    R.append(row("enqueue screen too large", "enqueue", BAD, T_ENQ_BAD, w=0x80000000, h=1))
    R.append(row("enqueue counts without DEVICE_PTRS", "enqueue", BAD, T_ENQ_DEV, count=True))
    R.append(row("enqueue null + counts", "enqueue", BAD, T_ENQ_NULL, args=False, count=True))
    return R


def test_call_contract_under_sanitizers(tmp_path):
    rows = table()
    path = tmp_path / "rows.tsv"
    path.write_text("\n".join(rows) + "\n")
    exe = tmp_path / "call_kat"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc"),
                    "-o", str(exe), os.path.join(HERE, "native", "call_kat_main.cpp")], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(rows)} rows, 0 mismatches" in r.stdout and "runtime error" not in r.stderr


def test_the_dispatch_source_routes_every_path_through_the_header():
    src = open(os.path.join(REPO, "truetrace-unity-pathtracer_amd", "csrc", "tt_dispatch.hip")).read()
    for name in ("kTrace", "kHeightmap", "kShadow", "kShadowHeightmap"):
        assert f"tt_call::{name}" in src, name
    assert src.count("tt_call::plan_call(") == 4 and src.count("tt_call::check_enqueue(") == 1
