"""include/zkpoa_merkle_paths.h against _abi.MERKLE_PATHS_SIGNATURES, as tests/test_audit_abi.py does for the verifier's
header: every prototype has an entry of the same shape, the library exports it, the main header includes the new one.
And what `merkle-tree --help` says of --any-order. No GPU."""
import os
import re
import subprocess

from conftest import ROOT


def test_merkle_paths_header_matches_the_binding_table(zk):
    from zkpoa_amd import _abi
    import test_abi
    src = open(os.path.join(ROOT, "include", "zkpoa_merkle_paths.h")).read()
    src = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", src)
    assert [n for _, n, _ in protos] == list(_abi.MERKLE_PATHS_SIGNATURES) and len(protos) == 4
    L = zk.lib()
    for ret, name, args in protos:
        restype, argtypes = _abi.signature(_abi.MERKLE_PATHS_SIGNATURES[name])
        assert test_abi._ctypes_class(restype) == test_abi._c_class(ret + " ret"), name
        assert [test_abi._ctypes_class(t) for t in argtypes] == [test_abi._c_class(a.strip()) for a in args.split(",")], name
        assert list(getattr(L, name).argtypes) == argtypes
    assert '#include "zkpoa_merkle_paths.h"' in open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    others = (_abi.SIGNATURES, _abi.LAYER_INPUT_SIGNATURES, _abi.SIGN_SIGNATURES, _abi.HD_SIGNATURES, _abi.AUDIT_SIGNATURES,
              _abi.HOOK_SIGNATURES)
    assert not any(set(_abi.MERKLE_PATHS_SIGNATURES) & set(t) for t in others)


def test_last_ms_knows_id_10_and_no_other_new_one(zk):
    """zkpoa_last_ms answers -1 for an id it does not have, and for no context at all: id 10 is read through a context
    on the GPU tests; here only that the range check moved by exactly one."""
    src = open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    assert re.search(r"\b10 = last zkpoa_anon_set_find_device, zkpoa_merkle_find, zkpoa_merkle_paths", src)
    assert zk.lib().zkpoa_last_ms(None, 10) == -1.0


def test_help_names_any_order(zk):
    rc = subprocess.run([zk.MERKLE_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 0
    assert ("Usage: merkle-tree --anon-set <FILE_PATH> --poa-input-data <FILE_PATH> --output-dir <DIR_PATH> [--any-order]"
            in rc.stdout)
    rc = subprocess.run([zk.MERKLE_BIN, "--any-order"], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 2 and "required arguments were not provided" in rc.stderr
