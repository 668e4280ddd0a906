"""include/zkpoa_state_proof.h against _abi.STATE_PROOF_SIGNATURES, as tests/test_audit_abi.py does for its header: every
prototype has a row of the same shape, the library exports it and lib() has applied the signature; the main header
includes the new one and declares nothing of it itself; the struct and the constants the binding states are the header's.
No GPU."""
import ctypes
import os
import re
import subprocess

from conftest import GOLDEN, ROOT


def header():
    return open(os.path.join(ROOT, "include", "zkpoa_state_proof.h")).read()


def test_header_matches_the_binding_table(zk):
    from zkpoa_amd import _abi
    import test_abi
    src = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", header(), flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \t*]+?[\s*])(zkpoa_\w+)\s*\(([^()]*)\)\s*;", src)
    assert [n for _, n, _ in protos] == list(_abi.STATE_PROOF_SIGNATURES) and len(protos) == 4
    L = zk.lib()
    for ret, name, args in protos:
        restype, argtypes = _abi.signature(_abi.STATE_PROOF_SIGNATURES[name])
        assert test_abi._ctypes_class(restype) == test_abi._c_class(ret + " ret"), name
        assert [test_abi._ctypes_class(t) for t in argtypes] == [test_abi._c_class(a.strip()) for a in args.split(",")], name
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes and fn.restype == restype, name
    main = open(os.path.join(ROOT, "include", "zkpoa_prover.h")).read()
    assert '#include "zkpoa_state_proof.h"' in main
    assert not any(re.search(r"\b%s\s*\(" % n, re.sub(r"/\*.*?\*/", "", main, flags=re.S)) for n in _abi.STATE_PROOF_SIGNATURES)
    others = (_abi.SIGNATURES, _abi.LAYER_INPUT_SIGNATURES, _abi.SIGN_SIGNATURES, _abi.HD_SIGNATURES, _abi.AUDIT_SIGNATURES,
              _abi.MERKLE_PATHS_SIGNATURES, _abi.SECP_PRIM_SIGNATURES, _abi.HOOK_SIGNATURES)
    assert not any(set(_abi.STATE_PROOF_SIGNATURES) & set(t) for t in others)


def test_constants_and_report_struct_are_the_headers(zk):
    import mpt_ref as m
    src = header()
    status = dict(re.findall(r"#define ZKPOA_MPT_(\w+)\s+(\d+)u", src))
    assert {k: int(v) for k, v in status.items()} == {
        "PRESENT": m.PRESENT, "ABSENT": m.ABSENT, "NO_NODES": m.NO_NODES, "HASH": m.HASH, "RLP": m.RLP, "CHILD": m.CHILD,
        "SHORT": m.SHORT, "LONG": m.LONG, "HEX_PREFIX": m.HEX_PREFIX, "ACCOUNT": m.ACCOUNT}
    assert len(zk.MPT_STATUS) == 10 and list(zk.MPT_STATUS) == m.STATUS_NAMES
    kinds = dict(re.findall(r"#define ZKPOA_MPT_(KEY32|ADDRESS20)\s+(\d+)\s", src))
    assert (int(kinds["KEY32"]), int(kinds["ADDRESS20"])) == (zk.MPT_KEY32, zk.MPT_ADDRESS20) == (0, 1)
    assert re.search(r"#define ZKPOA_ASSETS_STATE\s+0x10u", src) and zk.ASSETS_STATE == 0x10
    assert zk.ASSETS_STATE not in (zk.ASSETS_SET, zk.ASSETS_ROOT, zk.ASSETS_COMMITMENT, zk.ASSETS_PROOF)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} zkpoa_state_report;", src, flags=re.S).group(1), flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in zk.StateReport._fields_]
    assert ctypes.sizeof(zk.StateReport) == 9 * 8 + 4 * 4 + 8 + 32 + 8                 # the float and its padding


def test_incomplete_state_options_need_no_device(zk):
    if not os.path.exists(zk.AUDIT_BIN):
        import __graft_entry__ as entry
        entry.build()
    run_dir = os.path.join(GOLDEN, "ref", "1_sigs_1_batches_5_height__layer_three")
    base = [zk.AUDIT_BIN, "--anon-set", os.path.join(GOLDEN, "ref", "merkle", "anonymity_set_10.csv"), "--vkey",
            os.path.join(GOLDEN, "ref", "layer_three_vkey.json"), "--public", os.path.join(run_dir, "public.json"), "--proof",
            os.path.join(run_dir, "proof.json")]
    for extra in (["--state-proofs", "proofs.jsonl"], ["--state-root", "0x" + "00" * 32], ["--balance-unit", "gwei"]):
        rc = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert rc.returncode == 2 and rc.stdout == "" and "--state-proofs" in rc.stderr and "Usage: zkpoa-audit" in rc.stderr
    rc = subprocess.run([zk.AUDIT_BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 0 and "--state-proofs" in rc.stdout and "--block-header" in rc.stdout
