"""gemma_amd/csrc/host_linalg.h (the one small_inverse of the vc and mqs units) as a stand-alone host program,
tests/cpp/host_linalg_check.cpp: plain and under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp, flags=()):
    exe = os.path.join(str(tmp), "host_linalg_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "host_linalg_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr


def test_small_inverse_host_program(tmp_path):
    _build_and_run(tmp_path)


def test_small_inverse_host_program_under_sanitizers(tmp_path):
    """Its own main: no preloading.  Skipped only where g++ cannot link -fsanitize=address,undefined at all."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    _build_and_run(tmp_path, flags)
