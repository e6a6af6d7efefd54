"""The packed image's "same terms, same order" as a stand-alone program under AddressSanitizer and UBSan: tests/host/packed_image_main.cpp
runs the walks of k_assemble / k_assemble_sparse (gadfit_amd/csrc/packed_walk.h), the source lists of k_gather_sum
(packed_layout.cpp: build_gather_lists, summed by the kernel's own gather_sum) and a naive loop over the datasets on the host, on
random Gram images (gram_image.h) of a handful of small layouts, and compares every element bit for bit.  That these files need
neither a context nor a HIP header is part of what is tested.  No GPU, no library, nothing preloaded: one sanitized executable,
built with the clang that ships with ROCm."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')


@pytest.mark.skipif(not os.path.exists(CLANG), reason='no ROCm clang')
def test_packed_image_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'gadfit_amd', 'csrc')
    exe = str(tmp_path / 'packed_image_main')
    subprocess.run([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-Wall', '-I' + csrc,
                    os.path.join(ROOT, 'tests', 'host', 'packed_image_main.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ''
