"""gfh_debug_deferred without a GPU: the header declares it, the library exports it, gadfit_amd/_lib.py binds it, and a compile-only
context answers it -- nothing deferred, nothing owed -- while the library's symbol table stays exactly what the header declares."""
import ctypes
import os
import re
import shutil
import subprocess

from gadfit_amd import _lib
from gadfit_amd.ad import trace_model
from tests import models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'gadfit_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(gfh_[a-z0-9_]+)\s*\(', src)))


def test_compile_only_context_reports_the_declared_symbol_table():
    names = _declared()
    assert 'gfh_debug_deferred' in names and 'gfh_debug_deferred' in _lib.SYMBOLS
    c = _lib.Context(-1)
    try:
        c.set_model(trace_model(M.model_exp2, 4))
        assert c.debug_deferred() == dict(deferred=0, stored=0, materialised=0, owed=False)
        L = ctypes.CDLL(_lib.LIB_PATH)
        for n in names:
            assert hasattr(L, n), 'libgadfit_hip.so does not export ' + n
        assert sorted(_lib.SYMBOLS) == names
        nm = shutil.which('nm') or '/opt/rocm/lib/llvm/bin/llvm-nm'
        out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(l.split()[-1] for l in out.splitlines() if l.strip()) == names
    finally:
        c.close()


def test_group_of_compile_only_members_reports_member_zero():
    g = _lib.Context(devices=[-1, -1])
    try:
        assert g.debug_deferred() == dict(deferred=0, stored=0, materialised=0, owed=False)
    finally:
        g.close()
