"""The DepthNet entry points, which live beside the main table (paddle3d_amd._lib.DEPTHNET_ENTRY_POINTS, declared in
include/paddle3d_amd_depthnet.h): the library exports what the header declares, and the rows agree with their
declarations name for name and parameter for parameter -- what tests/test_abi.py asserts for ENTRY_POINTS and
paddle3d_amd.h.  The table is named in _lib.LAST_TABLES, a third tuple behind SIDE_TABLES and LATER_TABLES (which
tests/test_abi_cape.py and tests/test_abi_dcn.py pin): lib() and symbols(module) walk it last."""
import os
import re
import subprocess

import pytest

from test_abi import _ctype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "paddle3d_amd_depthnet.h")
MODULE = "test_memory_safety_depthnet_gpu"
NAMES = ("pd3_aspp_workspace", "pd3_aspp_forward", "pd3_depth_softmax_split")


@pytest.fixture(scope="module")
def built():
    from paddle3d_amd import build

    return build.build()


def test_rows_match_the_header_and_are_exported(built):
    from paddle3d_amd import _lib

    hdr = open(HEADER).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    declared = {name: (ret.strip(), [" ".join(q.split()) for q in params.split(",")])
                for ret, name, params in re.findall(r"([\w \*]+?)\b(pd3_\w+)\s*\(([^;{)]*)\)\s*;", hdr)}
    assert tuple(declared) == tuple(_lib.DEPTHNET_ENTRY_POINTS) == NAMES
    assert len(re.findall(r"\bpd3_\w+\s*\(", hdr)) == len(declared)  # nothing declared twice, nothing the pattern missed
    for other in ("paddle3d_amd.h", "paddle3d_amd_lanedet.h", "paddle3d_amd_cape.h", "paddle3d_amd_dcn.h"):
        text = open(os.path.join(ROOT, "include", other)).read()  # nor a declaration in two headers
        assert not [name for name in declared if re.search(r"\b" + name + r"\s*\(", text)], other
    out = subprocess.check_output(["nm", "-D", "--defined-only", built], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(declared) <= exported, set(declared) - exported
    L = _lib.lib()
    for name, (res, args, module) in _lib.DEPTHNET_ENTRY_POINTS.items():
        ret, params = declared[name]
        assert module == MODULE and os.path.isfile(os.path.join(ROOT, "tests", module + ".py"))
        assert res is _ctype(ret, returned=True), (name, ret, res)
        assert len(args) == len(params) == len(getattr(L, name).argtypes), (name, len(args), len(params))
        for i, (q, a) in enumerate(zip(params, args)):
            assert a is _ctype(q), (name, i, q, a)
    assert _lib.symbols(MODULE) == NAMES                                  # in order: what the guarded scenarios have to reach
    assert not set(_lib.symbols()) & set(_lib.DEPTHNET_ENTRY_POINTS)      # symbols() stays the main table


def test_last_tables_are_walked_behind_the_pinned_ones():
    """LAST_TABLES is walked by symbols(module) and lib(); every pinned value is what it was."""
    from paddle3d_amd import _lib

    assert _lib.LAST_TABLES == (_lib.DEPTHNET_ENTRY_POINTS,)
    assert _lib.LATER_TABLES == (_lib.DCN_ENTRY_POINTS,)
    assert _lib.SIDE_TABLES == (_lib.LANEDET_ENTRY_POINTS, _lib.CAPE_ENTRY_POINTS)
    assert _lib._tables() == (_lib.ENTRY_POINTS, *_lib.SIDE_TABLES)
    assert _lib.symbols() == tuple(_lib.ENTRY_POINTS) and len(_lib.ENTRY_POINTS) == 138
    earlier = (*_lib._tables(), *_lib.LATER_TABLES)
    assert not any(table is last for table in earlier for last in _lib.LAST_TABLES)
    assert _lib.symbols("test_memory_safety_dcn_gpu") == tuple(_lib.DCN_ENTRY_POINTS)
    L = _lib.lib()
    for table in _lib.LAST_TABLES:
        module = {row[2] for row in table.values()}
        assert len(module) == 1 and _lib.symbols(module.pop()) == tuple(table)
        for name, (res, args, _) in table.items():
            assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == list(args)


def test_no_name_sits_in_two_tables():
    from paddle3d_amd import _lib

    names = [name for table in (*_lib._tables(), *_lib.LATER_TABLES, *_lib.LAST_TABLES) for name in table]
    assert len(names) == len(set(names))
    modules = [{row[2] for row in table.values()} for table in (*_lib.SIDE_TABLES, *_lib.LATER_TABLES, *_lib.LAST_TABLES)]
    assert all(len(m) == 1 for m in modules) and len(set.union(*modules)) == len(modules)  # a module per table
    assert not set.union(*modules) & {row[2] for row in _lib.ENTRY_POINTS.values()}


def test_build_lists_the_header_and_the_source():
    from paddle3d_amd import build

    assert os.path.realpath(HEADER) in {os.path.realpath(h) for h in build._headers()}
    assert "depthnet.hip" in {os.path.basename(s) for s in build._sources()}
