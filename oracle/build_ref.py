"""TEST INFRASTRUCTURE -- builds oracle/_ref/libmgx_ref.so: the reference MGARD-X's own SERIAL
code path behind the C ABI of oracle/ref_driver.cpp (bound by oracle/ref.py).

Nothing of the reference is committed. Its checkout is found through MGARD_REFERENCE_DIR (default:
a directory ``reference`` next to this repository); the files cmake would generate from it (the
config header and the explicit-instantiation units) are generated here, into oracle/_ref/gen/, by
the rules the reference's own CMakeLists.txt files state. Where the checkout is absent the existing
oracle/_ref/ is kept as it is. The build is incremental: a second call compiles nothing.
"""
import concurrent.futures
import os
import re
import subprocess
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(REF_DIR, "libmgx_ref.so")
_GEN = os.path.join(REF_DIR, "gen")
_OBJ = os.path.join(REF_DIR, "obj")
_DRIVER = os.path.join(_HERE, "ref_driver.cpp")

CXX = os.environ.get("CXX", "g++")
CXXFLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]
DIMS = (1, 2, 3, 4, 5)
TYPES = (("float", "f32"), ("double", "f64"))
# cmake/MgardXGenerateSource.cmake: which dimensions each generator instantiates
_GENERATORS = {"AllCombinations": DIMS, "3D": (1, 2, 3), "ND": (4, 5)}
# the parts of src/mgard-x that Hierarchy, DataRefactor (both of its paths) and the SERIAL runtime need
_UNIT_DIRS = ("Hierarchy", "DataRefactoring/MultiDimension", "DataRefactoring/SingleDimension")
_PLAIN_SOURCES = ("Config/Config.cpp", "RuntimeX/DeviceAdapters/DeviceAdapterSerial.cpp",
                  "RuntimeX/AutoTuners/AutoTunerSerial.cpp", "RuntimeX/Utilities/Log.cpp")


def reference_dir():
    return os.environ.get("MGARD_REFERENCE_DIR",
                          os.path.join(os.path.dirname(_HERE), "..", "reference"))


def _write_if_changed(path, text):
    try:
        with open(path) as f:
            if f.read() == text:
                return
    except OSError:
        pass
    with open(path, "w") as f:
        f.write(text)


def _config_header(ref):
    """include/MGARDXConfig.h.in with #cmakedefine01: the SERIAL backend on, everything else off."""
    with open(os.path.join(ref, "include", "MGARDXConfig.h.in")) as f:
        text = f.read()
    text = re.sub(r"#cmakedefine01\s+(\w+)",
                  lambda m: "#define %s %d" % (m.group(1), m.group(1) == "MGARD_ENABLE_SERIAL"),
                  text)
    assert "#cmakedefine" not in text and not re.search(r"@\w+@", text)
    _write_if_changed(os.path.join(_GEN, "MGARDXConfig.h"), text)


def _units(ref):
    """(generated path, template path) of every SERIAL instantiation unit under _UNIT_DIRS, as the
    MgardXGenerateSource*() calls of the reference's CMakeLists.txt files list them."""
    out = []
    src = os.path.join(ref, "src", "mgard-x")
    for top in _UNIT_DIRS:
        for dirpath, _, files in os.walk(os.path.join(src, top)):
            if "CMakeLists.txt" not in files:
                continue
            with open(os.path.join(dirpath, "CMakeLists.txt")) as f:
                calls = re.findall(r'MgardXGenerateSource(\w+)\(\s*"(\w+)"\s*\)', f.read())
            rel = os.path.relpath(dirpath, src).replace(os.sep, "_")
            for kind, prefix in calls:
                template = os.path.join(dirpath, prefix + ".cpp.in")
                with open(template) as f:
                    body = f.read()
                for dim in _GENERATORS[kind]:
                    for ctype, _ in TYPES:
                        text = (body.replace("@NUM_DIM@", str(dim)).replace("@DATA_TYPE@", ctype)
                                .replace("@DEVICE_TYPE@", "SERIAL"))
                        name = "%s_%s_%dD_%s_SERIAL.cpp" % (rel, prefix, dim, ctype)
                        gen = os.path.join(_GEN, name)
                        _write_if_changed(gen, text)
                        out.append(gen)
    return out


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_ref(verbose=True, jobs=None):
    """Returns the library path, or None when neither a reference checkout nor a previous build
    is there."""
    ref = os.path.abspath(reference_dir())
    if not os.path.isdir(os.path.join(ref, "include", "mgard-x")):
        if verbose:
            print("oracle.build_ref: no reference checkout at %s (MGARD_REFERENCE_DIR); keeping %s"
                  % (ref, "the existing oracle/_ref" if os.path.exists(LIB_PATH) else "no build"))
        return LIB_PATH if os.path.exists(LIB_PATH) else None
    t0 = time.time()
    os.makedirs(_GEN, exist_ok=True)
    os.makedirs(_OBJ, exist_ok=True)
    _config_header(ref)
    inc = ["-I" + _GEN, "-I" + os.path.join(ref, "include")]
    cfg = os.path.join(_GEN, "MGARDXConfig.h")
    jobs_list = []  # (object, deps, command)
    for gen in _units(ref):
        obj = os.path.join(_OBJ, os.path.basename(gen)[:-4] + ".o")
        jobs_list.append((obj, [gen, cfg], [CXX] + CXXFLAGS + inc + ["-c", gen, "-o", obj]))
    for rel in _PLAIN_SOURCES:
        path = os.path.join(ref, "src", "mgard-x", rel)
        obj = os.path.join(_OBJ, rel.replace("/", "_")[:-4] + ".o")
        jobs_list.append((obj, [path, cfg], [CXX] + CXXFLAGS + inc + ["-c", path, "-o", obj]))
    for dim in DIMS:
        for ctype, short in TYPES:
            sfx = "%dd_%s" % (dim, short)
            obj = os.path.join(_OBJ, "ref_driver_%s.o" % sfx)
            jobs_list.append((obj, [_DRIVER, cfg], [CXX] + CXXFLAGS + inc + [
                "-DMGXR_D=%d" % dim, "-DMGXR_T=" + ctype, "-DMGXR_SFX=" + sfx,
                "-c", _DRIVER, "-o", obj]))
    todo = [j for j in jobs_list if _stale(j[0], j[1])]
    objs = [j[0] for j in jobs_list]
    if todo:
        n = jobs or min(16, os.cpu_count() or 1)
        if verbose:
            print("oracle.build_ref: compiling %d of %d units against %s (-j%d)"
                  % (len(todo), len(jobs_list), ref, n), flush=True)

        def run(job):
            r = subprocess.run(job[2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode:
                raise RuntimeError("oracle.build_ref: %s failed:\n%s" % (" ".join(job[2]), r.stdout))

        with concurrent.futures.ThreadPoolExecutor(n) as ex:
            list(ex.map(run, todo))
    if todo or _stale(LIB_PATH, objs):
        tmp = LIB_PATH + ".tmp"
        subprocess.check_call([CXX, "-shared", "-o", tmp] + objs + ["-lpthread"])
        os.replace(tmp, LIB_PATH)
        if verbose:
            print("oracle.build_ref: %s built in %.1f s" % (LIB_PATH, time.time() - t0))
    return LIB_PATH
