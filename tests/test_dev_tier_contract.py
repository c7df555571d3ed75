"""CPU (not gpu): every entry of the device tier opens on its context first.  Called with a NULL context and every
other argument zero / NULL, each dt_dev_* entry of the binding table answers DT_EINVAL and "invalid argument: ctx is
NULL" -- whatever scaffold it is written on -- and the table names every dt_dev_* entry the library defines."""
import ctypes as C
import os
import re

import pytest

from descriptools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_EINVAL = -1
DEV_ENTRIES = sorted(n for n in _lib._SIGS if n.startswith("dt_dev_"))


def test_binding_table_names_every_device_tier_entry():
    src = open(os.path.join(ROOT, "descriptools_amd", "csrc", "dt_capi.hip")).read()
    defined = re.findall(r'^extern "C" int (dt_dev_\w+)\(', src, re.M)
    assert len(defined) == len(set(defined))
    assert len(DEV_ENTRIES) == len(defined), sorted(set(defined) ^ set(DEV_ENTRIES))
    assert sorted(defined) == DEV_ENTRIES


@pytest.mark.parametrize("name", DEV_ENTRIES)
def test_null_context_is_refused_first(name):
    L = _lib.lib()
    _, argtypes = _lib._SIGS[name]
    rc = getattr(L, name)(*[t() for t in argtypes])   # a ctypes type called without a value is its zero / NULL
    assert rc == DT_EINVAL
    assert L.dt_last_error() == b"invalid argument: ctx is NULL"
