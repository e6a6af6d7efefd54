"""The host solver of the normal equations (gadfit_amd/csrc/normal_eq.cpp) as a stand-alone program under AddressSanitizer and UBSan:
tests/host/normal_eq_main.cpp factorises and solves at the sizes round the plain / blocked switch and the block edges, where the
blocked factorisation pads columns and an odd last row by repeating indices.  No GPU, no library, nothing preloaded: the two sources
are compiled into one sanitized executable with the clang that ships with ROCm (normal_eq.cpp uses ext_vector_type)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')


@pytest.mark.skipif(not os.path.exists(CLANG), reason='no ROCm clang')
def test_normal_eq_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'gadfit_amd', 'csrc')
    exe = str(tmp_path / 'normal_eq_main')
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-I' + csrc,
                    os.path.join(ROOT, 'tests', 'host', 'normal_eq_main.cpp'), os.path.join(csrc, 'normal_eq.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ''
