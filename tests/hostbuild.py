"""The tests' host compiles, in one place: the g++ shared-library builds of the files under
tests/hostsim/ (beside hostsim_lib's own), the stand-alone programs under the address and
undefined-behaviour sanitizers, and the checks of include/bmpc.h as C and as C++."""
import ctypes as C
import hashlib
import os
import subprocess

from common import HERE, PKG, REPO

INCLUDES = ["-I" + os.path.join(REPO, "include"), "-I" + os.path.join(PKG, "csrc")]
# one flag set for every library; -ffp-contract=off: the scene steps round every product before it is added
SHARED_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wno-unknown-pragmas"]
SANITIZE_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall",
                  "-Wno-unknown-pragmas"]
_libs = {}


def source_hash(sources, flags=()):
    """Hash of what a host build is compiled from: the sources, every csrc/*.h and tests/hostsim/*.h,
    include/bmpc.h and the flag set (the sidecar ``<so>.srchash`` records it: an mtime check would
    accept a stale binary)."""
    dirs = (os.path.join(PKG, "csrc"), os.path.join(HERE, "hostsim"))
    files = list(sources) + [os.path.join(d, f) for d in dirs for f in sorted(os.listdir(d)) if f.endswith(".h")]
    h = hashlib.sha256()
    for p in sorted(files + [os.path.join(REPO, "include", "bmpc.h")]):
        with open(p, "rb") as f:
            h.update(os.path.basename(p).encode() + b"\0" + f.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()[:16]


def shared(name, sources, flags=()):
    """tests/hostsim/libbmpc_hostsim_<name>.so built from `sources` (paths, or file names under
    tests/hostsim/), rebuilt when source_hash changes; the ctypes.CDLL, one per process."""
    if name not in _libs:
        sources = [s if os.path.isabs(s) else os.path.join(HERE, "hostsim", s) for s in sources]
        so = os.path.join(HERE, "hostsim", f"libbmpc_hostsim_{name}.so")
        stamp = so + ".srchash"
        cmd = ["g++", *SHARED_FLAGS, *flags, *INCLUDES]
        want = source_hash(sources, cmd)
        have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(so) else None
        if have != want:
            tmp = so + f".{os.getpid()}.tmp"
            subprocess.check_call(cmd + [*sources, "-o", tmp])
            os.replace(tmp, so)                      # atomic: concurrent test workers each build their own
            with open(stamp + f".{os.getpid()}", "w") as f:
                f.write(want + "\n")
            os.replace(stamp + f".{os.getpid()}", stamp)
        _libs[name] = C.CDLL(so)
    return _libs[name]


def sanitized_program(source, tmp_path, flags=()):
    """`source` (a path, or a file name under tests/hostsim/) as a stand-alone program compiled with
    -fsanitize=address,undefined and run once; the CompletedProcess."""
    source = source if os.path.isabs(source) else os.path.join(HERE, "hostsim", source)
    exe = tmp_path / os.path.splitext(os.path.basename(source))[0]
    cmd = ["g++", *SANITIZE_FLAGS, *flags, *INCLUDES, source, "-o", str(exe)]
    # the sanitizer runtimes linked into the program where the toolchain has them as archives (the
    # program then needs nothing of its environment's library order), else the shared ones
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def header_program(tmp_path, code, cxx=False):
    """The C program `code` compiled against include/bmpc.h with gcc and run: the integers it prints.
    cxx: the header also compiles alone as C++17, where its static_asserts are checked."""
    include = "-I" + os.path.join(REPO, "include")
    (tmp_path / "t.c").write_text(code)
    subprocess.check_call(["gcc", include, str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "t")]).decode().split()))
    if cxx:
        (tmp_path / "t.cpp").write_text('#include "bmpc.h"\nint main(){return 0;}\n')
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", include, str(tmp_path / "t.cpp")])
    return got
