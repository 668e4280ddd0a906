"""include/zkpoa_audit.h against _abi.AUDIT_SIGNATURES, as tests/test_abi.py does for the main header: every prototype
has an entry of the same shape, the library exports it, the main header includes the new one, and the struct the
binding declares is the header's. No GPU."""
import ctypes
import os
import re

from conftest import ROOT


def test_audit_header_matches_the_binding_table(zk):
    from zkpoa_amd import _abi
    import test_abi
    src = open(os.path.join(ROOT, "include", "zkpoa_audit.h")).read()
    src = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", src)
    assert [n for _, n, _ in protos] == list(_abi.AUDIT_SIGNATURES) and len(protos) == 4
    L = zk.lib()
    for ret, name, args in protos:
        restype, argtypes = _abi.signature(_abi.AUDIT_SIGNATURES[name])
        assert test_abi._ctypes_class(restype) == test_abi._c_class(ret + " ret"), name
        assert [test_abi._ctypes_class(t) for t in argtypes] == [test_abi._c_class(a.strip()) for a in args.split(",")], name
        assert list(getattr(L, name).argtypes) == argtypes
    assert '#include "zkpoa_audit.h"' in open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    others = (_abi.SIGNATURES, _abi.LAYER_INPUT_SIGNATURES, _abi.SIGN_SIGNATURES, _abi.HD_SIGNATURES, _abi.HOOK_SIGNATURES)
    assert not any(set(_abi.AUDIT_SIGNATURES) & set(t) for t in others)


def test_report_struct_and_masks_are_the_headers(zk):
    src = open(os.path.join(ROOT, "include", "zkpoa_audit.h")).read()
    masks = dict(re.findall(r"#define ZKPOA_ASSETS_(\w+)\s+0x(\w+)u", src))
    assert {k: int(v, 16) for k, v in masks.items()} == {"SET": zk.ASSETS_SET, "ROOT": zk.ASSETS_ROOT,
                                                         "COMMITMENT": zk.ASSETS_COMMITMENT, "PROOF": zk.ASSETS_PROOF}
    assert [f[0] for f in zk.AssetsReport._fields_] == ["root_le", "commitment", "rows", "duplicate_rows", "first_dup", "ascending"]
    assert ctypes.sizeof(zk.AssetsReport) == 32 + 32 + 8 + 8 + 16 + 8      # the int and its padding


def test_usage_error_needs_no_device(zk):
    """Missing arguments: exit 2 and nothing on stdout, before any device is asked for."""
    import subprocess
    if not os.path.exists(zk.AUDIT_BIN):
        import __graft_entry__ as entry
        entry.build()
    rc = subprocess.run([zk.AUDIT_BIN], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 2 and rc.stdout == "" and "--anon-set" in rc.stderr
