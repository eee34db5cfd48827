"""What the tests' helper programs share: building and loading the lane simulators of tests/hostsim (build_sim), the C++ mirror
programs of tests/cpp (build_mirror), the device probes of tests/backend (build_devprobe), its sanitized host-only programs (build_sanitized), the fake-JNI programs of tests/jni_stub (build_fake_jni) and the oracle's CPU harness; the
status constants of the C ABI; running a child script (run_child); and what the *_multidev_child.py scripts do alike (init_repeated,
slots, check_slots).  A plain module, imported by the test files and the child scripts."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (the child scripts import the package and the oracle from the repository root, as conftest.py lets the tests)
    sys.path.insert(0, ROOT)
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
SIM_FLAGS = ("-O2", "-std=c++17", "-fPIC", "-shared", "-pthread")

# ---- the C ABI's status values (include/lz4hip.h) ----
E_NO_DEVICE, E_ARG = -1, -3
LIB_ERROR = lambda status: -2 ** 31 + (-status)   # LZ4HIP_LIB_ERROR


def no_device():
    import torch
    return not torch.cuda.is_available()


# ---- builds ----
def newer_than(path, deps):
    """a dependency is missing or newer than `path` (which exists)"""
    t = os.path.getmtime(path)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def _sim_is_fresh(so, rec, cmd, extra_deps):
    try:
        with open(rec) as f:
            r = json.load(f)
        return r["cmd"] == cmd and not newer_than(so, [os.path.join(ROOT, d) for d in r["deps"]] + list(extra_deps))
    except (OSError, ValueError, KeyError, TypeError):
        return False


def build_sim(stem, variant="", flags=(), extra_deps=(), src_dir=HOSTSIM, out_dir=HOSTSIM):
    """<src_dir>/<stem>.cpp -> <out_dir>/lib<stem><variant>.so, loaded: SIM_FLAGS + flags for every simulator.  What the library was
    built from is the compiler's word (-MMD), kept beside it in lib<stem><variant>.so.d with the command line, every path relative to
    the repository root.  It is rebuilt when it or that record is missing or unreadable, a recorded file or one of extra_deps is
    missing or newer than it, or the command line is another one; the build goes to a temporary name and is moved into place, so a
    build cut short leaves no library.  (A library this process has loaded already stays the loaded one: dlopen goes by name.)"""
    rel = lambda p: os.path.relpath(str(p), ROOT)
    so = os.path.join(str(out_dir), "lib%s%s.so" % (stem, variant))
    rec = so + ".d"
    command = lambda out, dep: ["g++", *SIM_FLAGS, *flags, "-MMD", "-MF", rel(dep), "-o", rel(out), rel(os.path.join(str(src_dir), stem + ".cpp"))]
    cmd = command(so, rec)
    if not _sim_is_fresh(so, rec, cmd, extra_deps):
        tmp_so, tmp_rec = "%s.tmp%d" % (so, os.getpid()), "%s.tmp%d" % (rec, os.getpid())
        try:
            subprocess.check_call(command(tmp_so, tmp_rec), cwd=ROOT)
            with open(tmp_rec) as f:   # make's syntax: "<target>: <file> <file> \<newline> <file> ..."
                deps = f.read().replace("\\\n", " ").split(":", 1)[1].split()
            with open(tmp_rec, "w") as f:
                json.dump({"cmd": cmd, "deps": sorted({os.path.normpath(d) for d in deps})}, f, indent=1)
            if os.path.exists(rec):
                os.remove(rec)             # (no moment at which the new library stands beside the old record)
            os.replace(tmp_so, so)
            os.replace(tmp_rec, rec)
        finally:
            for t in (tmp_so, tmp_rec):
                if os.path.exists(t):
                    os.remove(t)
    return C.CDLL(so)


# ---- the device instantiation of the backend probes (tests/backend/devprobe.hip -> tests/backend/libdevprobe.so) ----
DEVPROBE_SO = os.path.join(ROOT, "tests", "backend", "libdevprobe.so")
DEVPROBE_DEPS = ("tests/backend/devprobe.hip", "tests/backend/probes.h", "lz4-java_amd/csrc/wave_dev.h", "lz4-java_amd/csrc/group_dev.h")


def build_devprobe():
    """tests/backend/libdevprobe.so, loaded: rebuilt when a dependency is newer (or it is missing) and hipcc exists, otherwise what
    build() of __graft_entry__.py made.  With neither a library nor hipcc: an AssertionError that names build() -- not a skip."""
    import __graft_entry__ as entry        # (the recipe is build()'s: one command line in one place)
    stale = not os.path.exists(DEVPROBE_SO) or newer_than(DEVPROBE_SO, [os.path.join(ROOT, d) for d in DEVPROBE_DEPS])
    if stale and entry.find_hipcc():
        entry.compile_devprobe()
    assert os.path.exists(DEVPROBE_SO), ("tests/backend/libdevprobe.so is missing and there is no hipcc to build it: "
                                         "run build() of __graft_entry__.py where ROCm is installed (python -c 'import __graft_entry__ as g; g.build()')")
    return C.CDLL(DEVPROBE_SO)


def _link_lz4hip():
    d = os.path.join(ROOT, "lz4-java_amd")
    return ["-L" + d, "-llz4hip", "-Wl,-rpath," + d, "-Wl,-rpath,/opt/rocm/lib"]


def build_mirror(name, out_dir, werror=False, src=None):
    """tests/cpp/<name>.cpp (or the source file `src`), linked with liblz4hip.so -> the executable <out_dir>/<name>; returns its path"""
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + (["-Werror"] if werror else []) +
                          ["-I" + ROOT, str(src or os.path.join(ROOT, "tests", "cpp", name + ".cpp"))] + _link_lz4hip() + ["-o", exe])
    return exe


def build_sanitized(name, out_dir):
    """tests/cpp/<name>.cpp, a stand-alone program of host code alone (no library, no device), with the address and undefined-behaviour
    sanitizers, every finding fatal -> the executable <out_dir>/<name>; returns its path"""
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def build_fake_jni(name, out_dir):
    """tests/jni_stub/<name>.c + the shim (malloc / free counted) -> the executable <out_dir>/<name>; returns its path"""
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "jni_stub", "build.sh"), name, str(out_dir)])
    return os.path.join(str(out_dir), name)


def typecheck_jni_shim():
    """the JNI shim type-checks against the stub jni.h of tests/jni_stub (no JDK needed)"""
    subprocess.check_call(["gcc", "-fsyntax-only", "-Wall", "-std=c11", "-I" + os.path.join(ROOT, "tests", "jni_stub"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "lz4-java_amd", "jni", "net_jpountz_lz4_LZ4HIPJNI.c")])


def build_cpu_bench(exe):
    """oracle/cpu_bench.c (the CPU leg of the benchmark) -> the executable `exe`"""
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-o", exe, os.path.join(ROOT, "oracle", "cpu_bench.c"), "-ldl", "-lpthread"])


# ---- child processes ----
def run_child(script, *args, timeout):
    """runs tests/<script> with this interpreter; exit status 0 or an AssertionError with the tails of its output; returns stdout"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script)] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return p.stdout


# ---- inside a *_multidev_child.py ----
def package():
    """-> (amd, L): the Python package and its ctypes library, no device initialised"""
    import importlib
    amd = importlib.import_module("lz4-java_amd")
    return amd, amd.lib()


def init_devices(ids):
    """lz4hip_init on this device list -> (amd, L)"""
    amd, L = package()
    assert L.lz4hip_init((C.c_int * len(ids))(*ids), len(ids)) == 0, L.lz4hip_last_error()
    assert L.lz4hip_device_count() == len(ids)
    return amd, L


def init_repeated(D):
    """lz4hip_init([0] * D): device 0 listed D times, so that the host batches take the multi-device branch on one GPU -> (amd, L)"""
    return init_devices([0] * D)


def offsets(sizes):
    """where each of consecutive pieces of these sizes starts"""
    import numpy as np
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)


def slots(srcs, caps, guard=8):
    """-> (source offsets of the joined srcs, offsets of destination slots of caps[i] + guard bytes, the 0xEE-filled destination)"""
    return offsets([len(s) for s in srcs]), offsets([c + guard for c in caps]), bytearray(b"\xee" * (int(sum(caps)) + guard * len(caps)))


def check_slots(out, dst, dst_off, caps, want, srcs, tag=(), extra=lambda i: (), guard=8):
    """per block against want[i] = (result, bytes): the result, the bytes, and 0xEE from the result's end to the end of the slot's guard"""
    for i, (r, by) in enumerate(want):
        assert int(out[i]) == r, ("result",) + tuple(tag) + (i, len(srcs[i])) + tuple(extra(i)) + (caps[i], int(out[i]), r)
        o, n = int(dst_off[i]), max(r, 0)
        assert bytes(dst[o:o + n]) == by, ("bytes",) + tuple(tag) + (i,)
        assert dst[o + n:o + caps[i] + guard] == b"\xee" * (caps[i] + guard - n), ("written past the result",) + tuple(tag) + (i,)
