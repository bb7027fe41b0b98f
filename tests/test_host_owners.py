"""The host-side owners of orb_slam_amd/csrc/orbx_host.h without a GPU: tests/_probe/host_owners.cpp drives them against a stand-in HIP
runtime (tests/_probe/hip_stub) under AddressSanitizer + UndefinedBehaviorSanitizer: staging offsets and alignment, and that a failed
allocation or creation leaves an empty owner behind, with nothing leaked or freed twice."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_owners(tmp_path):
    exe = str(tmp_path / "host_owners")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "host_owners.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host owners ok" in r.stdout
