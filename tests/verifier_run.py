"""Builds and runs one of the host verifiers (tools/verify_*.cpp) for the
test_*_host.py files. No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the store's source, for the verifiers that build stores through the C API
STORE_SRC = os.path.join("filodb_amd", "csrc", "chunk_builder.cpp")


def run_verifier(tool, tmp_dir, flags=(), sources=(), args=(), key="class"):
    """Compiles tools/<tool>.cpp (plus `sources`, paths from the repository
    root) with -O2 -std=c++17 and `flags` into tmp_dir, runs it with `args`
    and prints what it wrote. Returns (returncode, stdout, rows): rows maps
    the name of every "<key>=<name> k=v ..." line of stdout to {k: int(v)}.

    The compiler is a host C++ compiler; with `sources`, hipcc, only for the
    HIP include path the store's header wants."""
    if sources:
        cxx = shutil.which("hipcc") or os.path.join(
            os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        assert os.path.exists(cxx), "no hipcc"
    else:
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler"
    exe = str(tmp_dir / tool)
    subprocess.run([cxx, "-O2", "-std=c++17", *flags, "-o", exe,
                    os.path.join(REPO, "tools", tool + ".cpp"),
                    *(os.path.join(REPO, s) for s in sources)], check=True)
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    print(p.stdout)
    print(p.stderr)
    rows = {}
    for m in re.finditer(rf"^{key}=(\w+)((?: \w+=\d+)+)$", p.stdout, re.M):
        rows[m.group(1)] = {k: int(v) for k, v in
                            (kv.split("=") for kv in m.group(2).split())}
    return p.returncode, p.stdout, rows
