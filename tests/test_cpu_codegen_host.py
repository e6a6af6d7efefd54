"""The generator (gadfit_amd/csrc/codegen.cpp, emit_*.cpp, ws_plan.cpp) with model.cpp and device_text.cpp as a stand-alone program
under AddressSanitizer and UBSan: tests/host/codegen_main.cpp builds three tapes by hand -- every elemental, an integrate() with a
finite and an infinite bound, two variants split by one guard -- and generates their sources in the default form, with finite
differences and (the first) with the batch kernels, plus two refusals.  That these files need neither a context nor a HIP header is
part of what is tested.  No GPU, no library, nothing preloaded: one sanitized executable, built with the clang that ships with ROCm
(device_text.cpp uses #embed)."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')


@pytest.mark.skipif(not os.path.exists(CLANG), reason='no ROCm clang')
def test_codegen_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'gadfit_amd', 'csrc')
    sources = sorted(glob.glob(os.path.join(csrc, 'emit_*.cpp'))) + [os.path.join(csrc, f) for f in ('codegen.cpp', 'ws_plan.cpp', 'model.cpp', 'device_text.cpp')]
    sources.append(os.path.join(ROOT, 'tests', 'host', 'codegen_main.cpp'))
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-Wno-c23-extensions', '-I' + csrc]

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + '.o'))
        subprocess.run([CLANG] + flags + ['-c', src, '-o', obj], check=True)
        return obj
    with ThreadPoolExecutor(max_workers=8) as pool:          # (the objects side by side: the unroller alone is half the time)
        objs = list(pool.map(compile_one, sources))
    exe = str(tmp_path / 'codegen_main')
    subprocess.run([CLANG, '-fsanitize=address,undefined'] + objs + ['-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == ''
