"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/rlhip.h declares; calls fail loudly (no CPU fallback) when no GPU is present."""
import ctypes as C
import os
import re

import pytest

from ranklib_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ensure_built():
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_library_exports_every_declared_symbol():
    _ensure_built()
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    declared = sorted(set(re.findall(r"\b(rl_[a-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations found"
    L = C.CDLL(N.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), "librlhip.so does not export %s" % name
    assert sorted(N.ABI_SYMBOLS) == declared
    assert L.rl_abi_version() == 5


def test_launch_arm_indices_of_the_python_side_are_the_headers():
    """RL_ARR_LAUNCH_ARMS is read by index: _native.ARM / HARM must name exactly the RL_ARM_* / RL_HARM_* values of include/rlhip.h, the array id
    is appended behind the existing ones, and no earlier id has moved"""
    hdr = open(os.path.join(ROOT, "include", "rlhip.h")).read()
    for prefix, table in (("RL_ARM_", N.ARM), ("RL_HARM_", N.HARM)):
        got = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b%s([A-Z0-9_]+) = (\d+)" % prefix, hdr)}
        assert got == table, (prefix, sorted(set(got.items()) ^ set(table.items())))
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bRL_ARR_([A-Z0-9_]+) = (\d+)", hdr)}
    assert ids == N.ARR and len(set(ids.values())) == len(ids)
    assert ids["LAUNCH_ARMS"] == max(ids.values()) == 25 and ids["PIECE_STATS"] == 24 and ids["STEP_LOG"] == 20 and ids["LAMBDA"] == 1
    # the counters fit between the last arm and the settings, nothing overlaps
    idx = sorted(v for k, v in N.ARM.items() if k not in ("HIST_ROOT", "HIST_CHILD", "COUNT_"))
    assert len(set(idx)) == len(idx) and idx[0] >= N.ARM["HIST_CHILD"] + N.HARM["COUNT_"] and idx[-1] < N.ARM["COUNT_"]


def test_no_cpu_fallback_without_device(gpu_available):
    _ensure_built()
    if gpu_available:
        pytest.skip("GPU present")
    assert N.device_count() == 0
    with pytest.raises(N.RankLibError) as e:
        N.Trainer(n_trees=1)
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(N.RankLibError):
        N.Model("<ensemble>\n</ensemble>\n")


def test_parameter_validation_messages():
    _ensure_built()
    L = N.lib()
    p = N.RlParams()
    L.rl_params_default(C.byref(p))
    # defaults of learning/tree/LambdaMART.java:37-42
    assert (p.n_trees, p.n_leaves, p.n_threshold, p.min_leaf_support, p.early_stop_rounds, p.metric_k) == \
        (1000, 10, 256, 1, 100, 10)
    assert abs(p.learning_rate - 0.1) < 1e-8
    h = C.c_void_p()
    p.n_trees = 0
    assert L.rl_create(C.byref(p), C.byref(h)) == -1
    assert b"n_trees" in L.rl_last_error()


def test_header_is_valid_c99_and_the_c_example_compiles(tmp_path):
    """the boundary is a C ABI: rlhip.h must compile as plain C (no C++ types), and the example that drives the whole path from C
    (integration/c/train_example.c) must compile against it; with a GPU it is also linked and run"""
    import shutil
    import subprocess
    cc = shutil.which("gcc")
    assert cc, "gcc is part of the image"
    inc = os.path.join(ROOT, "include")
    src = os.path.join(ROOT, "integration", "c", "train_example.c")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c", os.path.join(inc, "rlhip.h")])
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, src])


@pytest.mark.gpu
def test_c_example_trains_through_the_abi(tmp_path):
    import subprocess
    _ensure_built()
    exe = str(tmp_path / "train_example")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "c", "train_example.c"),
                           "-L", libdir, "-lrlhip", "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "## LambdaMART" in out.stdout and "<ensemble>" in out.stdout and out.stdout.count("<tree id=") == 10


# ---- the JNI shim (integration/jni/RlHipNative.c): no JDK in this image, so no build -- but it can be TYPE-checked --------------------
def test_jni_shim_type_checks_against_the_jni_signatures(tmp_path):
    """gcc -fsyntax-only against tests/stubs/jni.h, a minimal stand-in that declares the JNINativeInterface_ entries the shim calls with the
    signatures of the JNI specification, and against include/rlhip.h: wrong argument counts / types on either side fail here"""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "integration", "jni", "RlHipNative.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_java_native_declarations_match_the_shim():
    """every `static native` of RlHipNative.java has its Java_<class>_<method> in the shim with JNIEnv*, jclass and the mapped parameter
    types in order (a mismatch is an UnsatisfiedLinkError or a corrupted call at run time, not a compile error, on the Java side)"""
    import re
    java = open(os.path.join(ROOT, "integration", "java", "ciir", "umass", "edu", "learning", "tree", "RlHipNative.java")).read()
    csrc = open(os.path.join(ROOT, "integration", "jni", "RlHipNative.c")).read()
    tmap = {"long": "jlong", "int": "jint", "float": "jfloat", "boolean": "jboolean", "double": "jdouble", "FloatBuffer": "jobject",
            "float[]": "jfloatArray", "int[]": "jintArray", "double[]": "jdoubleArray", "void": "void"}
    decls = re.findall(r"static\s+native\s+([\w\[\]]+)\s+(\w+)\s*\(([^)]*)\)\s*;", java, re.S)
    assert len(decls) >= 8
    for ret, name, args in decls:
        want = ["JNIEnv *", "jclass"] + [tmap[" ".join(a.split()[:-1])] for a in args.split(",") if a.strip()]
        m = re.search(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+Java_ciir_umass_edu_learning_tree_RlHipNative_%s\s*\(([^)]*)\)" % name, csrc, re.S)
        assert m, "no JNI entry point for " + name
        assert m.group(1) == tmap[ret], (name, m.group(1), ret)
        got = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            got.append("JNIEnv *" if a.startswith("JNIEnv") else a.rsplit(" ", 1)[0])
        assert got == want, (name, got, want)
