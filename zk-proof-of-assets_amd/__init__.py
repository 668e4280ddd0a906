"""zkpoa_amd -- Python host layer over libzkpoa_prover.so (the MI355X Groth16 prover).

Mirrors the reference's interface for the prove step: the reference calls an external prover
as `prover <zkey> <wtns> <proof.json> <public.json>` (scripts/g16_prove.sh:248-252) or
`snarkjs groth16 prove` with the same four arguments (scripts/g16_prove.sh:255-259); here
that is `groth16_prove(zkey_path, wtns_path, proof_path, public_path)`, plus the stages of
the path (`msm_g1`, `msm_g2`, `ntt`, `h_scalars`) as the C ABI exposes them.

This package never computes on the CPU: if the shared library is missing, or no HIP device
is usable, calls raise. (The directory name has a hyphen, so the package is loaded through
`__graft_entry__.load_package()` / tests/conftest.py under the module name `zkpoa_amd`.)
"""
import ctypes
import os

from ._abi import (EXPORTS, LIB_PATH, PROVER_ERROR, PROVER_ERROR_RUNTIME, PROVER_ERROR_SHORT_BUFFER,  # noqa: F401
                   PROVER_INVALID_WITNESS_LENGTH, PROVER_OK, ZkpoaError, _buf, _name, _Out, _replace_file, _scalar,
                   _sized, lib)

_HERE = os.path.dirname(os.path.abspath(__file__))
PROVER_BIN = os.path.join(_HERE, "prover")
MERKLE_BIN = os.path.join(_HERE, "merkle-tree")
AUDIT_BIN = os.path.join(_HERE, "zkpoa-audit")
SIGS_BIN = os.path.join(_HERE, "ecdsa-sigs-parser")
SETUP_BIN = os.path.join(_HERE, "zkpoa-setup")
VERIFY_BIN = os.path.join(_HERE, "zkpoa-verify")
SANITIZE_BIN = os.path.join(_HERE, "zkpoa-sanitize")

# the bits of zkpoa_zkey_verify's result (include/zkpoa_prover.h ZKPOA_ZKEY_*)
ZKEY_CHECKS = {"HEADER": 0x01, "POINTS": 0x02, "DELTA": 0x04, "COEFFS": 0x08, "A": 0x10, "B1": 0x20, "B2": 0x40,
               "ICCH": 0x80, "CSHASH": 0x100, "CONTRIBUTIONS": 0x200}
SETUP_TRANSCRIPT = 0x1      # zkpoa_zkey_new_ex: fill in section 10's circuit hash (ZKPOA_SETUP_TRANSCRIPT)
# the bits of zkpoa_ptau_verify's result (include/zkpoa_prover.h ZKPOA_PTAU_*)
PTAU_CHECKS = {"POINTS": 0x001, "TAU_G1": 0x002, "TAU_G2": 0x004, "ALPHA": 0x008, "BETA": 0x010,
               "LAGRANGE_TAU_G1": 0x020, "LAGRANGE_TAU_G2": 0x040, "LAGRANGE_ALPHA": 0x080, "LAGRANGE_BETA": 0x100,
               "CONTRIBUTIONS": 0x200}


def shard_flags(split=False, block_log=0):
    """include/zkpoa_prover.h: ZKPOA_SHARD_SPLIT_CHAIN | ZKPOA_SHARD_BLOCK_CYCLIC(block_log)."""
    return (1 if split else 0) | ((int(block_log) & 0xff) << 8)


ASSETS_SET, ASSETS_ROOT, ASSETS_COMMITMENT, ASSETS_PROOF = 1, 2, 4, 8   # Context.assets_verify's failed checks


class AssetsReport(ctypes.Structure):
    """zkpoa_assets_report of include/zkpoa_audit.h"""
    _fields_ = [("root_le", ctypes.c_uint8 * 32), ("commitment", ctypes.c_uint8 * 32), ("rows", ctypes.c_uint64),
                ("duplicate_rows", ctypes.c_uint64), ("first_dup", ctypes.c_uint64 * 2), ("ascending", ctypes.c_int)]


ASSETS_STATE = 0x10                     # include/zkpoa_state_proof.h: the set against an Ethereum state root
MPT_KEY32, MPT_ADDRESS20 = 0, 1         # Context.mpt_verify's key kinds
MPT_STATUS = ("present", "absent", "no nodes", "hash", "rlp", "child", "short", "long", "hex-prefix", "account")


class StateReport(ctypes.Structure):
    """zkpoa_state_report of include/zkpoa_state_proof.h"""
    _fields_ = [("rows", ctypes.c_uint64), ("proven_present", ctypes.c_uint64), ("proven_absent", ctypes.c_uint64),
                ("rows_without_proof", ctypes.c_uint64), ("rows_failed", ctypes.c_uint64), ("rows_differ", ctypes.c_uint64),
                ("proofs_read", ctypes.c_uint64), ("proofs_not_in_set", ctypes.c_uint64), ("first_bad_row", ctypes.c_uint64),
                ("first_bad_kind", ctypes.c_uint32), ("first_bad_status", ctypes.c_uint32), ("first_bad_where", ctypes.c_uint32),
                ("first_diff_absent", ctypes.c_uint32), ("first_diff_row", ctypes.c_uint64),
                ("first_diff_chain_balance32", ctypes.c_uint8 * 32), ("kernel_ms", ctypes.c_float)]


def _node_args(nodes, node_offset, node_length, first_node):
    """The node arguments of include/zkpoa_state_proof.h from bytes and three integer sequences -> (ctypes arguments,
    keepalives)"""
    import numpy as np
    off = np.ascontiguousarray(node_offset, dtype=np.uint64)
    length = np.ascontiguousarray(node_length, dtype=np.uint32)
    first = np.ascontiguousarray(first_node, dtype=np.uint64)
    pn, kn = _buf(bytes(nodes) if len(nodes) else b"\0")
    as_ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    return ((pn, len(nodes), as_ptr(off, ctypes.c_uint64), as_ptr(length, ctypes.c_uint32), as_ptr(first, ctypes.c_uint64)),
            (kn, off, length, first))


class Context:
    """A device context (one GPU). Raises if no HIP device is usable."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = lib().zkpoa_context_create(device, ctypes.byref(self._h), err, 512)
        if rc != PROVER_OK:
            self._h = None
            raise ZkpoaError("zkpoa_context_create: " + err.value.decode())

    def close(self):
        if self._h:
            lib().zkpoa_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != PROVER_OK:
            raise ZkpoaError("%s failed (%d): %s" % (what, rc, lib().zkpoa_last_error(self._h).decode()))

    def stream(self, lane=0):
        """The HIP stream of a lane as an integer handle (wrap with torch.cuda.ExternalStream to order torch work /
        RCCL collectives with the library's kernels without host synchronisation)."""
        h = int(lib().zkpoa_context_stream(self._h, lane) or 0)
        if h == 0:      # 0 would silently become the legacy default stream in torch.cuda.ExternalStream
            raise ZkpoaError("zkpoa_context_stream: no stream for lane %d" % lane)
        return h

    def synchronize(self):
        """Wait for lane 0's stream (the split-chain stages only enqueue)."""
        self._check(lib().zkpoa_context_synchronize(self._h), "zkpoa_context_synchronize")

    def set_option(self, key, value):
        self._check(lib().zkpoa_set_option(self._h, key.encode(), int(value)), "zkpoa_set_option")

    def msm_points_limit(self):
        """Points one MSM of this context sorts at once right now: 2^27 until a lane's workspace did not fit in HBM (or
        under option lane_workspace_max_mb), then the size that did (include/zkpoa_prover.h, "Memory pressure")."""
        return int(lib().zkpoa_msm_points_limit(self._h))

    def last_ms(self, ident):
        return float(lib().zkpoa_last_ms(self._h, ident))

    # ---- stages, host buffers -------------------------------------------------------------
    def msm_g1(self, bases, scalars, n=None):
        n = len(scalars) // 32 if n is None else n
        pb, kb = _buf(bases)
        ps, ks = _buf(scalars)
        out = ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_msm_g1(self._h, pb, ps, n, out), "zkpoa_msm_g1")
        return out.raw

    def msm_g2(self, bases, scalars, n=None):
        n = len(scalars) // 32 if n is None else n
        pb, kb = _buf(bases)
        ps, ks = _buf(scalars)
        out = ctypes.create_string_buffer(128)
        self._check(lib().zkpoa_msm_g2(self._h, pb, ps, n, out), "zkpoa_msm_g2")
        return out.raw

    def ntt(self, data, log_n, inverse=False):
        buf = bytearray(data)
        p, k = _buf(buf)
        self._check(lib().zkpoa_ntt(self._h, p, log_n, 1 if inverse else 0), "zkpoa_ntt")
        return bytes(buf)

    def h_scalars(self, coeffs_section, witness, n_vars, log_domain):
        pc, kc = _buf(coeffs_section)
        pw, kw = _buf(witness)
        out = ctypes.create_string_buffer(32 << log_domain)
        self._check(lib().zkpoa_h_scalars(self._h, pc, len(coeffs_section), pw, n_vars, log_domain, out),
                    "zkpoa_h_scalars")
        return out.raw

    # ---- stages, device pointers (ints) ---------------------------------------------------
    def msm_g1_device(self, d_bases, d_scalars, n):
        out = ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_msm_g1_device(self._h, d_bases, d_scalars, n, out), "zkpoa_msm_g1_device")
        return out.raw

    def msm_g1_device_lane(self, lane, d_bases, d_scalars, n):
        """G1 MSM on lane `lane` (own stream + workspace); thread-safe across different lanes."""
        out = ctypes.create_string_buffer(64)
        if lib().zkpoa_msm_g1_device_lane(self._h, lane, d_bases, d_scalars, n, out) != PROVER_OK:
            raise ZkpoaError("zkpoa_msm_g1_device_lane failed")
        return out.raw

    def last_ms_lane(self, lane, ident):
        return float(lib().zkpoa_last_ms_lane(self._h, lane, ident))

    # ---- the anonymity-set Merkle tree (scripts/merkle_tree.rs) ---------------------------------------------------
    def poseidon2(self, left, right):
        """n independent circomlib Poseidon(2) hashes; left, right: n x 32 B LE standard form -> n x 32 B."""
        n = len(left) // 32
        pl, kl = _buf(left)
        pr, kr = _buf(right)
        out = _Out(32 * n)
        self._check(lib().zkpoa_poseidon2(self._h, pl, pr, n, out), "zkpoa_poseidon2")
        return out.bytes()

    def poseidon2_device(self, d_left, d_right, n, d_out):
        self._check(lib().zkpoa_poseidon2_device(self._h, d_left, d_right, n, d_out), "zkpoa_poseidon2_device")

    # ---- one item per lane: the calls of include/zkpoa_prover.h and include/zkpoa_ecdsa_sign.h below --------------------
    def _lanes(self, name, args, out_sizes):
        """The C function `name`(handle, *args, *outputs): the bytes-like ones among args go over as buffers, the integers
        as they are, and there is one output buffer per size -> the outputs' bytes, in order."""
        ins = [a if isinstance(a, int) else _buf(bytes(a)) for a in args]
        outs = [_Out(k) for k in out_sizes]
        self._check(getattr(lib(), name)(self._h, *([a if isinstance(a, int) else a[0] for a in ins] + outs)), name)
        return tuple(o.bytes() for o in outs)

    def _hashes(self, name, messages, length):
        n, data = (len(messages) // length, messages) if length else (int(messages), b"")
        return self._lanes(name, (data, length, n), [32 * n])[0]

    # ---- ECDSA -> ECDSA* (scripts/ecdsa_sigs_parser.ts): 32-byte integers big-endian ------------------------------
    def ecdsa_star(self, r, s, msghash, v, addresses):
        """n signatures: r, s, msghash n x 32 B big-endian, v n bytes, addresses n x 20 B ->
        (r' n x 32 B, keys n x 64 B (x || y), derived addresses n x 20 B, status bytes); include/zkpoa_prover.h."""
        n = len(v)
        if len(r) != 32 * n or len(s) != 32 * n or len(msghash) != 32 * n or len(addresses) != 20 * n:
            raise ZkpoaError("ecdsa_star: the arrays do not describe %d signatures" % n)
        return self._lanes("zkpoa_ecdsa_star", (n, r, s, msghash, v, addresses), [32 * n, 64 * n, 20 * n, n])

    def keccak256(self, messages, length):
        """Keccak-256 of len(messages) / length messages of `length` bytes packed back to back (length 0: pass n)."""
        return self._hashes("zkpoa_keccak256", messages, length)

    def eth_address(self, pubkeys):
        """ethers.computeAddress for n x 64 B keys (x || y big-endian) -> (n x 20 B, list of n EIP-55 strings)."""
        n = len(pubkeys) // 64
        addr, text = self._lanes("zkpoa_eth_address", (pubkeys, n), [20 * n, 42 * n])
        chars = text.decode()
        return addr, [chars[42 * i:42 * i + 42] for i in range(n)]

    # ---- signing (tests/generate_ecdsa_signatures.ts): include/zkpoa_ecdsa_sign.h; 32-byte integers big-endian -----
    def sha256(self, messages, length):
        """SHA-256 of len(messages) / length messages of `length` bytes packed back to back (length 0: pass n)."""
        return self._hashes("zkpoa_sha256_batch", messages, length)

    def secp256k1_pubkey(self, seckeys):
        """n x 32 B keys -> (keys n x 64 B (x || y), addresses n x 20 B, status bytes: 1 = key zero or not below n)."""
        n = len(seckeys) // 32
        return self._lanes("zkpoa_secp256k1_pubkey", (n, seckeys), [64 * n, 20 * n, n])

    def secp256k1_derive_keys(self, seed, first, n):
        """The n keys (SHA-256(seed || be64(i)) mod (n - 1)) + 1 for i = first ..: n x 32 B."""
        return self._lanes("zkpoa_secp256k1_derive_keys", (seed, len(seed), first, n), [32 * n])[0]

    def rfc6979_nonce(self, seckeys, msghash, skip=0):
        """The RFC 6979 candidate after `skip` refusals for n keys and n hashes (n x 32 B each) -> n x 32 B."""
        n = len(seckeys) // 32
        if len(msghash) != 32 * n:
            raise ZkpoaError("rfc6979_nonce: %d keys need as many hashes" % n)
        return self._lanes("zkpoa_rfc6979_nonce", (n, seckeys, msghash, skip), [32 * n])[0]

    def ecdsa_sign(self, seckeys, msghash, stride=None):
        """n signatures with RFC 6979 nonces and low s. msghash: 32 B for all keys or n x 32 B (stride: 0 / 32, by default
        told from its length) -> (r, s n x 32 B, v n bytes, keys n x 64 B, addresses n x 20 B, status bytes)."""
        n = len(seckeys) // 32
        if stride is None:
            stride = 0 if len(msghash) == 32 and n != 1 else 32
        if stride in (0, 32) and len(msghash) != (32 * n if stride else 32):
            raise ZkpoaError("ecdsa_sign: the hashes do not fit %d keys with stride %d" % (n, stride))
        return self._lanes("zkpoa_ecdsa_sign", (n, seckeys, msghash, stride), [32 * n, 32 * n, n, 64 * n, 20 * n, n])

    # ---- HD-wallet key sources (BIP-32): include/zkpoa_hd_wallet.h; 32-byte integers big-endian, keys as 33 B key data --
    def sha512(self, messages, length):
        """SHA-512 of len(messages) / length messages of `length` bytes packed back to back (length 0: pass n) -> n x 64 B."""
        n, data = (len(messages) // length, messages) if length else (int(messages), b"")
        return self._lanes("zkpoa_sha512_batch", (data, length, n), [64 * n])[0]

    def hmac_sha512(self, key, messages, length):
        """HMAC-SHA512 of such a batch under one key of any length -> n x 64 B."""
        n, data = (len(messages) // length, messages) if length else (int(messages), b"")
        return self._lanes("zkpoa_hmac_sha512_batch", (key, len(key), data, length, n), [64 * n])[0]

    def bip32_children(self, parent_key, chain, first, n):
        """Children first .. first + n - 1 of one parent (33 B key data: 00 || k or 02 / 03 || x; 32 B chain code) ->
        (key data n x 33 B, chain codes n x 32 B, keys n x 64 B (x || y), addresses n x 20 B, status bytes: 1 = BIP-32's
        invalid child). A public parent with a hardened index in the range raises."""
        if len(parent_key) != 33 or len(chain) != 32:
            raise ZkpoaError("bip32_children: the parent is 33 B of key data and a 32 B chain code")
        return self._lanes("zkpoa_bip32_children", (parent_key, chain, first, n), [33 * n, 32 * n, 64 * n, 20 * n, n])

    def bip32_tweak(self, parent_key, tweaks):
        """The child-key step after its HMAC, for n tweaks IL (n x 32 B) -> (key data, keys, addresses, status bytes)."""
        n = len(tweaks) // 32
        if len(parent_key) != 33:
            raise ZkpoaError("bip32_tweak: the parent is 33 B of key data")
        return self._lanes("zkpoa_bip32_tweak", (parent_key, n, tweaks), [33 * n, 64 * n, 20 * n, n])

    def bip32_derive_path(self, key, chain, path):
        """The key at `path` ("m/44'/60'/0'/0") below (key data, chain code) -> (key data, chain code)."""
        if len(key) != 33 or len(chain) != 32:
            raise ZkpoaError("bip32_derive_path: the key is 33 B of key data and a 32 B chain code")
        ins = [_buf(bytes(key)), _buf(bytes(chain))]
        outs = [_Out(33), _Out(32)]
        self._check(lib().zkpoa_bip32_derive_path(self._h, ins[0][0], ins[1][0], path.encode(), *outs), "zkpoa_bip32_derive_path")
        return outs[0].bytes(), outs[1].bytes()

    def merkle_build(self, addresses, balances, device=False, n=None):
        """Tree over (address, balance) pairs: host buffers (n x 32 B LE each) or, with device=True, device pointers."""
        return MerkleTree(self, addresses, balances, device, n)

    def anon_set_index(self, d_addresses, n, d_perm):
        """d_perm[0..n) (u32, device) <- the row numbers of the n device-resident 32-byte keys ordered by (key, row): a
        stable sort, exact for every input."""
        self._check(lib().zkpoa_anon_set_index_device(self._h, d_addresses, n, d_perm), "zkpoa_anon_set_index_device")

    def anon_set_find(self, d_keys, n, d_perm, d_queries, m, d_first, d_count):
        """Lookup through the stable index (all device pointers): d_count[i] <- the rows whose key equals query i,
        d_first[i] <- the lowest of them, 0xFFFFFFFF when there is none. d_keys, d_perm: as anon_set_index took and left them."""
        self._check(lib().zkpoa_anon_set_find_device(self._h, d_keys, n, d_perm, d_queries, m, d_first, d_count),
                    "zkpoa_anon_set_find_device")

    def anon_set_audit(self, addresses, n=None):
        """The duplicate check of a published set's addresses (host buffer, n x 32 B LE) -> (rows that repeat an earlier
        row's address, the pair (i, j) with the smallest such j or None, is the file strictly ascending)."""
        n = len(addresses) // 32 if n is None else n
        p, keep = _buf(addresses)
        out = (ctypes.c_uint64 * 4)()
        self._check(lib().zkpoa_anon_set_audit(self._h, p, n, out), "zkpoa_anon_set_audit")
        return int(out[0]), ((int(out[1]), int(out[2])) if out[0] else None), bool(out[3])

    def assets_verify(self, addresses, balances, vkey_json, public_json, proof_json, expected_commitment=None, n=None):
        """The verifier's whole check -> (failed checks: a mask of ASSETS_SET / ROOT / COMMITMENT / PROOF, report dict);
        every check runs whatever the others found. Raises on malformed JSON or a set value that is no field element."""
        n = len(addresses) // 32 if n is None else n
        pa, ka = _buf(addresses)
        pb, kb = _buf(balances)
        failed = ctypes.c_uint32(0)
        rep = AssetsReport()
        self._check(lib().zkpoa_assets_verify(self._h, pa, pb, n, vkey_json.encode(), public_json.encode(), proof_json.encode(),
                                              None if expected_commitment is None else _buf(bytes(expected_commitment))[0],
                                              ctypes.byref(failed), ctypes.addressof(rep)), "zkpoa_assets_verify")
        return int(failed.value), {
            "root": int.from_bytes(bytes(rep.root_le), "little"), "commitment": bytes(rep.commitment), "rows": int(rep.rows),
            "duplicate_rows": int(rep.duplicate_rows),
            "first_dup": (int(rep.first_dup[0]), int(rep.first_dup[1])) if rep.duplicate_rows else None,
            "ascending": bool(rep.ascending)}

    # ---- the set against an Ethereum state root (include/zkpoa_state_proof.h) ------------------------------------------
    def mpt_verify(self, keys, root, nodes, node_offset, node_length, first_node, key_kind=MPT_KEY32):
        """Merkle-Patricia proofs of n keys (n x 32 B, or n x 20 B addresses with key_kind=MPT_ADDRESS20) under `root`:
        the nodes in one 8-aligned blob with their offsets and lengths, first_node[i] .. first_node[i + 1] those of item
        i, root first -> (status bytes, where: numpy uint32, value spans: numpy uint64 [n, 2] = offset into nodes, length)."""
        import numpy as np
        n = len(first_node) - 1
        if len(keys) != n * (20 if key_kind == MPT_ADDRESS20 else 32) or len(root) != 32:
            raise ZkpoaError("mpt_verify: the keys and first_node do not describe the same number of items")
        args, keep = _node_args(nodes, node_offset, node_length, first_node)
        status, where, span = _Out(n), np.zeros(max(n, 1), dtype=np.uint32), np.zeros((max(n, 1), 2), dtype=np.uint64)
        self._check(lib().zkpoa_mpt_verify(self._h, n, _buf(bytes(keys) or b"\0")[0], key_kind, bytes(root), *args, status,
                                           where.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                           span.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "zkpoa_mpt_verify")
        return status.bytes(), where[:n], span[:n]

    def eth_account_proofs(self, addresses, root, nodes, node_offset, node_length, first_node, with_hashes=True):
        """Account proofs (what eth_getProof returns) of n x 20 B addresses under a state root -> (status bytes, where,
        nonces: numpy uint64, balances n x 32 B big-endian, storage roots, code hashes (n x 32 B each, None without
        with_hashes)); all zero unless the status is 0."""
        import numpy as np
        n = len(first_node) - 1
        if len(addresses) != 20 * n or len(root) != 32:
            raise ZkpoaError("eth_account_proofs: the addresses and first_node do not describe the same number of items")
        args, keep = _node_args(nodes, node_offset, node_length, first_node)
        status, where, nonce = _Out(n), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64)
        balance, sroot, code = _Out(32 * n), _Out(32 * n) if with_hashes else None, _Out(32 * n) if with_hashes else None
        self._check(lib().zkpoa_eth_account_proofs(self._h, n, _buf(bytes(addresses) or b"\0")[0], bytes(root), *args, status,
                                                   where.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                   nonce.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), balance, sroot, code),
                    "zkpoa_eth_account_proofs")
        return (status.bytes(), where[:n], nonce[:n], balance.bytes(), sroot.bytes() if with_hashes else None,
                code.bytes() if with_hashes else None)

    def anon_set_state_check(self, addresses, balances, proofs_path, root, unit_divisor=1, n=None):
        """The whole check of a set (host buffers, n x 32 B LE each) against a JSON Lines file of eth_getProof results
        under a state root -> a dict of zkpoa_state_report's fields, with "ok": every row has a valid proof that gives
        its balance. Raises only for an unreadable or malformed file."""
        n = len(addresses) // 32 if n is None else n
        pa, ka = _buf(addresses if len(addresses) else b"\0")
        pb, kb = _buf(balances if len(balances) else b"\0")
        rep = StateReport()
        self._check(lib().zkpoa_anon_set_state_check_file(self._h, pa, pb, n, os.fsencode(proofs_path), bytes(root), unit_divisor,
                                                          ctypes.addressof(rep)), "zkpoa_anon_set_state_check_file")
        none = (1 << 64) - 1
        out = {name: int(getattr(rep, name)) for name, _ in StateReport._fields_[:8]}
        out.update(ok=rep.first_bad_row == none, first_bad_row=None if rep.first_bad_row == none else int(rep.first_bad_row),
                   first_bad_kind=int(rep.first_bad_kind), first_bad_status=int(rep.first_bad_status),
                   first_bad_where=int(rep.first_bad_where), first_diff_absent=bool(rep.first_diff_absent),
                   first_diff_row=None if rep.first_diff_row == none else int(rep.first_diff_row),
                   first_diff_chain_balance=int.from_bytes(bytes(rep.first_diff_chain_balance32), "big"),
                   kernel_ms=float(rep.kernel_ms))
        return out

    def msm_table(self, group, d_bases, n, window_bits=0):
        """Fixed-base table over n device-resident bases (group 1 = G1, 2 = G2) -> MsmTable."""
        return MsmTable(self, group, d_bases, n, window_bits)

    def msm_table_run(self, table, d_scalars, lane=0):
        """sum k_i P_i over a table's bases, fixed-base form; thread-safe across different lanes."""
        out = ctypes.create_string_buffer(64 if table.group == 1 else 128)
        if lib().zkpoa_msm_table_run_lane(self._h, lane, table._h, d_scalars, out) != PROVER_OK:
            raise ZkpoaError("zkpoa_msm_table_run_lane failed")
        return out.raw

    def msm_g2_device(self, d_bases, d_scalars, n):
        out = ctypes.create_string_buffer(128)
        self._check(lib().zkpoa_msm_g2_device(self._h, d_bases, d_scalars, n, out), "zkpoa_msm_g2_device")
        return out.raw

    def ntt_device(self, d_data, log_n, inverse=False):
        self._check(lib().zkpoa_ntt_device(self._h, d_data, log_n, 1 if inverse else 0), "zkpoa_ntt_device")

    def gen_bases_g1_device(self, a, b, i0, n, d_out):
        self._check(lib().zkpoa_gen_bases_g1_device(self._h, _scalar(a), _scalar(b), i0, n, d_out),
                    "zkpoa_gen_bases_g1_device")

    def gen_bases_g2_device(self, a, b, i0, n, d_out):
        self._check(lib().zkpoa_gen_bases_g2_device(self._h, _scalar(a), _scalar(b), i0, n, d_out),
                    "zkpoa_gen_bases_g2_device")

    # ---- element-wise hooks ------------------------------------------------------------------
    def field_op(self, field, op, a, b=None):
        n = len(a) // 32
        pa, ka = _buf(a)
        pb, kb = _buf(b) if b is not None else (None, None)
        out = _Out(32 * n)
        self._check(lib().zkpoa_field_op(self._h, field, op, pa, pb, out, n), "zkpoa_field_op")
        return out.bytes()

    def group_add(self, group, a, b):
        size = 64 if group == 1 else 128
        n = len(a) // size
        pa, ka = _buf(a)
        pb, kb = _buf(b)
        out = _Out(size * n)
        self._check(lib().zkpoa_group_add(self._h, group, pa, pb, out, n), "zkpoa_group_add")
        return out.bytes()

    def field_prim(self, field, op, operands, n_out=1, raw=True):
        """zkpoa_field_prim: `operands` is the list of the op's operand arrays (n elements each, 32 B or 64 B for
        Fq2); returns the list of its `n_out` result arrays."""
        size = 64 if field == 2 else 32
        n = len(operands[0]) // size if operands else 0
        assert all(len(x) == n * size for x in operands)
        pin, kin = _buf(b"".join(operands))
        out = _Out(size * n * n_out)
        self._check(lib().zkpoa_field_prim(self._h, field, op, pin, out, n, 1 if raw else 0), "zkpoa_field_prim")
        res = out.bytes()
        return [res[size * n * j:size * n * (j + 1)] for j in range(n_out)]

    def curve_prim(self, group, op, a=None, b=None, k=None, n=None):
        """zkpoa_curve_prim: a, b as the op takes them (XYZZ / affine bytes), k a sequence of u32; returns n XYZZ."""
        fb = 32 if group == 1 else 64
        if n is None:
            n = len(a) // (4 * fb) if a is not None else len(b) // (2 * fb)
        pa, ka = _buf(a) if a is not None else (None, None)
        pb, kb = _buf(b) if b is not None else (None, None)
        pk, kk = _buf(b"".join(int(v).to_bytes(4, "little") for v in k)) if k is not None else (None, None)
        out = _Out(4 * fb * n)
        self._check(lib().zkpoa_curve_prim(self._h, group, op, pa, pb, pk, out, n), "zkpoa_curve_prim")
        return out.bytes()

    def fq29_prim(self, op, data, n, out_words, raw=True):
        """zkpoa_fq29_prim: `data` holds the n records of the op (32-bit words, little-endian); returns the n result
        records of `out_words` words each, as bytes."""
        pin, kin = _buf(data)
        out = _Out(4 * out_words * n)
        self._check(lib().zkpoa_fq29_prim(self._h, op, pin, out, n, 1 if raw else 0), "zkpoa_fq29_prim")
        return out.bytes()

    def secp_prim(self, op, data, n, out_words):
        """zkpoa_secp_prim: `data` holds the op's operand arrays back to back (n values of eight little-endian 32-bit
        words each); returns its result arrays likewise, `out_words` words per record in all, as bytes."""
        pin, kin = _buf(data)
        out = _Out(4 * out_words * n)
        self._check(lib().zkpoa_secp_prim(self._h, op, pin, out, n), "zkpoa_secp_prim")
        return out.bytes()

    def test_msm_sort(self, scalars, n, c=0, merged=False, for_g2=False, density=None, k0=0, lane=0, caps=None):
        """zkpoa_test_msm_sort: phase A of one MSM request on host scalars -> a dict with "plan" (the thirteen words of
        zkpoa_test_msm_plan), "total_entries", "max_count", "total1", and counts, off0, po_a, sorted, pbkt, order,
        len_hist as bytes of 32-bit words. caps: the seven capacities in words (default: each array's upper bound)."""
        dens = (ctypes.c_double * 32)(*density) if density is not None else None
        plan = (ctypes.c_uint64 * 13)()
        if lib().zkpoa_test_msm_plan(n, c, int(merged), int(for_g2), dens, k0, plan, 13) != 13:
            raise ZkpoaError("zkpoa_test_msm_plan: arguments out of range")
        W, TB, K0 = plan[1], plan[4], plan[5]
        if caps is None:        # every piece holds an entry, every entry is one of the n * W digits
            caps = [TB, TB + 1, TB + 1, n * W, n * W, n * W, K0 + 1]
        bufs = [(ctypes.c_uint32 * max(1, k))() for k in caps]
        out = (ctypes.c_void_p * 7)(*[ctypes.addressof(b) for b in bufs])
        totals = (ctypes.c_uint32 * 3)()
        ps, ks = _buf(scalars)
        rc = lib().zkpoa_test_msm_sort(self._h, lane, ps, n, c, int(merged), int(for_g2), dens, k0, plan, totals, out,
                                       (ctypes.c_uint64 * 7)(*caps))
        if rc != PROVER_OK:
            raise ZkpoaError("zkpoa_test_msm_sort failed (%d)" % rc)
        sizes = [TB, TB + 1, TB + 1, totals[0], totals[2], totals[2], K0 + 1]
        res = {"plan": list(plan), "total_entries": totals[0], "max_count": totals[1], "total1": totals[2]}
        for name, b, k in zip(("counts", "off0", "po_a", "sorted", "pbkt", "order", "len_hist"), bufs, sizes):
            res[name] = bytes(memoryview(b).cast("B")[:4 * k])
        return res

    def test_msm_density(self, scalars, n):
        """zkpoa_test_msm_density: the 32 doubles the prover's density measurement gives for n host scalars."""
        out = (ctypes.c_double * 32)()
        ps, ks = _buf(scalars)
        self._check(lib().zkpoa_test_msm_density(self._h, ps, n, out), "zkpoa_test_msm_density")
        return list(out)

    def ntt_form(self, data, log_n, form, inverse=False, batch=1, stride=None):
        """zkpoa_ntt_form: form 0 = DIF (natural in, bit-reversed out), 1 = DIT (bit-reversed in, natural out), 2 = to the
        odd coset; `batch` vectors of 2^log_n elements, `stride` elements apart (default 2^log_n), transformed in a copy
        of `data`, which is returned whole (the elements between the vectors included)."""
        buf = bytearray(data)
        p, k = _buf(buf)
        stride = (1 << log_n) if stride is None else stride
        if batch >= 1 and log_n <= 28 and len(buf) < ((batch - 1) * stride + (1 << log_n)) * 32:
            raise ValueError("ntt_form: data is shorter than ((batch - 1) * stride + 2^log_n) * 32 bytes")
        self._check(lib().zkpoa_ntt_form(self._h, p, log_n, form, 1 if inverse else 0, batch, stride), "zkpoa_ntt_form")
        return bytes(buf)

    # ---- proving key + prove -----------------------------------------------------------------
    def load_zkey(self, zkey_bytes):
        return ZKey(self, zkey_bytes)

    def load_zkey_device(self, n_vars, n_public, log_domain, d_A, d_B1, d_B2, d_C, d_H, d_coefs, n_coefs,
                         header_points):
        """Proving key from device-resident sections (device pointers as ints); the caller keeps them alive."""
        return ZKey._adopt(self, lib().zkpoa_zkey_load_device, n_vars, n_public, log_domain, d_A, d_B1, d_B2, d_C, d_H,
                           d_coefs, n_coefs, bytes(header_points))

    def setup_accumulate(self, group, d_points, n_points, d_coefs, d_point_index, d_signal, nnz, n_signals, d_out):
        """out[s] = sum of coefs[e] * points[point_index[e]] over the entries of signal s (device pointers as ints):
        one zkey point section of `snarkjs zkey new` (include/zkpoa_prover.h: zkpoa_setup_accumulate)."""
        self._check(lib().zkpoa_setup_accumulate(self._h, group, d_points, n_points, d_coefs, d_point_index, d_signal,
                                                 nnz, n_signals, d_out), "zkpoa_setup_accumulate")

    def zkey_new(self, r1cs_path, ptau_path, zkey_path):
        """`snarkjs zkey new` on files (include/zkpoa_prover.h: zkpoa_zkey_new)."""
        self._check(lib().zkpoa_zkey_new(self._h, os.fsencode(r1cs_path), os.fsencode(ptau_path),
                                         os.fsencode(zkey_path)), "zkpoa_zkey_new")

    def wtns_check(self, r1cs_path, wtns_path):
        """`snarkjs wtns check`: -> (number of violated constraints, smallest violated index or None)."""
        bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(lib().zkpoa_wtns_check(self._h, os.fsencode(r1cs_path), os.fsencode(wtns_path), ctypes.byref(bad),
                                           ctypes.byref(first)), "zkpoa_wtns_check")
        return int(bad.value), (int(first.value) if bad.value else None)

    def zkey_verify(self, r1cs_path, ptau_path, zkey_path):
        """`snarkjs zkey verify` on files: -> the bitmask of failed checks (ZKEY_CHECKS), 0 = the key belongs to this
        circuit and this ceremony. A malformed file raises ZkpoaError (include/zkpoa_prover.h: zkpoa_zkey_verify)."""
        failed = ctypes.c_uint32(0)
        self._check(lib().zkpoa_zkey_verify(self._h, os.fsencode(r1cs_path), os.fsencode(ptau_path),
                                            os.fsencode(zkey_path), ctypes.byref(failed)), "zkpoa_zkey_verify")
        return int(failed.value)

    def ptau_verify(self, path, piece_points=0):
        """`snarkjs powersoftau verify` on a .ptau: -> (bitmask of failed checks (PTAU_CHECKS), 0 = good;
        (power, ceremony power, prepared, contributions)). piece_points: points per upload (0 = derived from free HBM).
        A malformed file raises ZkpoaError (include/zkpoa_prover.h: zkpoa_ptau_verify)."""
        failed, info = ctypes.c_uint32(0), (ctypes.c_uint32 * 4)()
        self._check(lib().zkpoa_ptau_verify(self._h, os.fsencode(path), int(piece_points), ctypes.byref(failed), info),
                    "zkpoa_ptau_verify")
        return int(failed.value), tuple(int(v) for v in info)

    def ec_intt(self, group, d_in, log_n, d_out):
        """Inverse NTT over 2^log_n curve points of G1 (group 1) or G2 (2), device pointers as ints, wire format:
        out[j] = sum_i (w_n^(-ij) / n) * in[i]; d_out may equal d_in (include/zkpoa_prover.h: zkpoa_ec_intt_device)."""
        self._check(lib().zkpoa_ec_intt_device(self._h, group, d_in, log_n, d_out), "zkpoa_ec_intt_device")

    def ptau_prepare_phase2(self, in_path, out_path):
        """`snarkjs powersoftau prepare phase2` on files: writes out_path with sections 12-15 made from sections 2-5
        -> (power, ceremony power, the input was prepared already, contributions). A malformed file raises ZkpoaError
        and leaves nothing at out_path (include/zkpoa_prover.h: zkpoa_ptau_prepare_phase2)."""
        info = (ctypes.c_uint32 * 4)()
        self._check(lib().zkpoa_ptau_prepare_phase2(self._h, os.fsencode(in_path), os.fsencode(out_path), info),
                    "zkpoa_ptau_prepare_phase2")
        return tuple(int(v) for v in info)

    def zkey_contribute(self, zkey_in_path, zkey_out_path, delta=None):
        """The arithmetic of `snarkjs zkey contribute` (delta: int in [1, r), None = random)."""
        self._check(lib().zkpoa_zkey_contribute(self._h, os.fsencode(zkey_in_path), os.fsencode(zkey_out_path),
                                                _scalar(delta)), "zkpoa_zkey_contribute")

    def zkey_new_ex(self, r1cs_path, ptau_path, zkey_path, flags=SETUP_TRANSCRIPT):
        """`zkey new` with section 10's circuit hash filled in (include/zkpoa_prover.h: zkpoa_zkey_new_ex)."""
        self._check(lib().zkpoa_zkey_new_ex(self._h, os.fsencode(r1cs_path), os.fsencode(ptau_path),
                                            os.fsencode(zkey_path), flags), "zkpoa_zkey_new_ex")

    def zkey_contribute_ex(self, zkey_in_path, zkey_out_path, delta=None, name=None):
        """`zkey contribute` on a key with a transcript: the arithmetic and a contribution record."""
        self._check(lib().zkpoa_zkey_contribute_ex(self._h, os.fsencode(zkey_in_path), os.fsencode(zkey_out_path),
                                                   _scalar(delta), _name(name)), "zkpoa_zkey_contribute_ex")

    def zkey_beacon(self, zkey_in_path, zkey_out_path, beacon, num_iterations_exp, name=None):
        """`snarkjs zkey beacon`: beacon bytes, 2^num_iterations_exp SHA-256 iterations (at most 2^30)."""
        self._check(lib().zkpoa_zkey_beacon(self._h, os.fsencode(zkey_in_path), os.fsencode(zkey_out_path), bytes(beacon),
                                            len(beacon), num_iterations_exp, _name(name)), "zkpoa_zkey_beacon")

    def hash_form(self, group, points, piece_points=0):
        """Hash form of wire-form points, converted on the device in pieces: -> (bytes, Blake2b-512 digest)."""
        unit = 64 if group == 1 else 128
        n = len(points) // unit
        out, dg = _Out(n * unit), ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_hash_form(self._h, group, bytes(points), n, piece_points, out, dg), "zkpoa_hash_form")
        return out.bytes(), dg.raw

    def compressed_form(self, group, points, piece_points=0):
        """Compressed form of wire-form points, converted on the device in pieces: -> (bytes, Blake2b-512 digest)."""
        unit = 64 if group == 1 else 128
        n = len(points) // unit
        out, dg = _Out(n * unit // 2), ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_compressed_form(self._h, group, bytes(points), n, piece_points, out, dg),
                    "zkpoa_compressed_form")
        return out.bytes(), dg.raw

    def scalar_mul_each(self, group, d_points, d_scalars, n, d_out):
        """d_out[i] = k_i * P_i over n points of G1 (group 1) or G2 (2): device pointers as ints, points in wire format,
        scalars 32 B little-endian below r (include/zkpoa_prover.h: zkpoa_scalar_mul_each_device)."""
        self._check(lib().zkpoa_scalar_mul_each_device(self._h, group, d_points, d_scalars, n, d_out),
                    "zkpoa_scalar_mul_each_device")

    def power_scalars(self, first, ratio, i0, n, d_out):
        """d_out[i] = first * ratio^(i0 + i), i < n, 32 B little-endian (device pointer as int)."""
        self._check(lib().zkpoa_power_scalars_device(self._h, _scalar(first), _scalar(ratio), i0, n, d_out),
                    "zkpoa_power_scalars_device")

    def ptau_new(self, power, out_path):
        """`snarkjs powersoftau new bn128 <power> <out>`: every point the generator, no contribution record."""
        self._check(lib().zkpoa_ptau_new(self._h, power, os.fsencode(out_path)), "zkpoa_ptau_new")

    def ptau_contribute(self, in_path, out_path, secrets=None, name=None):
        """`snarkjs powersoftau contribute`: secrets = (tau, alpha, beta), ints in [1, r), None = random; appends a
        record to section 7 (include/zkpoa_prover.h: zkpoa_ptau_contribute)."""
        sec = None if secrets is None else b"".join(_scalar(x) for x in secrets)
        self._check(lib().zkpoa_ptau_contribute(self._h, os.fsencode(in_path), os.fsencode(out_path), sec, _name(name)),
                    "zkpoa_ptau_contribute")

    def ptau_beacon(self, in_path, out_path, beacon, num_iterations_exp, name=None):
        """`snarkjs powersoftau beacon`: beacon bytes, 2^num_iterations_exp SHA-256 iterations (at most 2^30)."""
        self._check(lib().zkpoa_ptau_beacon(self._h, os.fsencode(in_path), os.fsencode(out_path), bytes(beacon),
                                            len(beacon), num_iterations_exp, _name(name)), "zkpoa_ptau_beacon")

    def sqrt_device(self, field, a):
        """Square roots on the device: a = n elements of Fq (field 0, 32 B each) or Fq2 (field 2, 64 B) in wire form ->
        (roots, flags): the non-negative root of each element (all-zero when it is no square) and one 0/1 byte each."""
        size = 64 if field == 2 else 32
        n = len(a) // size
        roots, ok = _Out(n * size), _Out(n)
        self._check(lib().zkpoa_sqrt_device(self._h, field, bytes(a), n, roots, ok), "zkpoa_sqrt_device")
        return roots.bytes(), ok.bytes()

    def decompressed_form(self, group, data, piece_points=0):
        """Compressed form (32 B per G1 point, 64 B per G2 point) -> wire-form points, on the device in pieces; a point
        that does not decompress raises ZkpoaError naming its index."""
        unit = 64 if group == 1 else 128
        n = len(data) // (unit // 2)
        out = _Out(n * unit)
        self._check(lib().zkpoa_decompressed_form(self._h, group, bytes(data), n, piece_points, out),
                    "zkpoa_decompressed_form")
        return out.bytes()

    def from_hash_form(self, group, data, piece_points=0):
        """Hash form -> wire-form points, on the device in pieces; a point that is not in hash form raises ZkpoaError
        naming its index."""
        unit = 64 if group == 1 else 128
        n = len(data) // unit
        out = _Out(n * unit)
        self._check(lib().zkpoa_from_hash_form(self._h, group, bytes(data), n, piece_points, out), "zkpoa_from_hash_form")
        return out.bytes()

    def ptau_export_challenge(self, ptau_path, challenge_path):
        """`snarkjs powersoftau export challenge`: writes the challenge file -> its Blake2b-512, the file's challenge."""
        h = ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_ptau_export_challenge(self._h, os.fsencode(ptau_path), os.fsencode(challenge_path), h),
                    "zkpoa_ptau_export_challenge")
        return h.raw

    def ptau_challenge_contribute(self, challenge_path, response_path, secrets=None):
        """`snarkjs powersoftau challenge contribute`: secrets as ptau_contribute -> the response file's Blake2b-512."""
        sec = None if secrets is None else b"".join(_scalar(x) for x in secrets)
        h = ctypes.create_string_buffer(64)
        self._check(lib().zkpoa_ptau_challenge_contribute(self._h, os.fsencode(challenge_path),
                                                          os.fsencode(response_path), sec, h),
                    "zkpoa_ptau_challenge_contribute")
        return h.raw

    def ptau_import_response(self, old_path, response_path, new_path, name=None):
        """`snarkjs powersoftau import response`: the response's sections and one more record into new_path."""
        self._check(lib().zkpoa_ptau_import_response(self._h, os.fsencode(old_path), os.fsencode(response_path),
                                                     os.fsencode(new_path), _name(name)), "zkpoa_ptau_import_response")

    def h_diff(self, points, n):
        """points[i + n] - points[i], i < n - 1, over 2n - 1 wire-form G1 points (device)."""
        out = ctypes.create_string_buffer((n - 1) * 64)
        self._check(lib().zkpoa_h_diff(self._h, bytes(points), n, out), "zkpoa_h_diff")
        return out.raw

    def load_zkey_device_shard(self, n_vars, n_public, log_domain, rank, world, split, d_A, d_B1, d_B2, d_C, d_H,
                               d_coefs, n_coefs, header_points, block_log=0):
        """Shard `rank` of `world` from device-resident sections that hold only this rank's ranges -- or, with
        block_log = L > 0, its blocks of 2^L items (block b to rank b mod world) concatenated
        (include/zkpoa_prover.h: zkpoa_zkey_load_device_shard, ZKPOA_SHARD_*); the caller keeps the buffers alive."""
        return ZKey._adopt(self, lib().zkpoa_zkey_load_device_shard, n_vars, n_public, log_domain, rank, world,
                           shard_flags(split, block_log), d_A, d_B1, d_B2, d_C, d_H, d_coefs, n_coefs, bytes(header_points))

    def load_zkey_shard(self, zkey_bytes, rank, world):
        """Shard `rank` of `world` of a proving key: only that byte range of sections 5-9 is uploaded."""
        p, k = _buf(zkey_bytes)
        return ZKey._adopt(self, lib().zkpoa_zkey_load_shard, p, len(zkey_bytes), rank, world)

    def load_zkey_shard_ex(self, zkey_bytes, rank, world, split=False, block_log=0):
        """Shard `rank` of `world` with shard flags (include/zkpoa_prover.h ZKPOA_SHARD_*): `split` = the H-scalar chain
        is split too; block_log = L > 0 = sections 5-8 dealt out in blocks of 2^L items instead of one range per rank
        (what the prover's own multi-GPU path, env ZKPOA_DEVICES, loads)."""
        p, k = _buf(zkey_bytes)
        return ZKey._adopt(self, lib().zkpoa_zkey_load_shard_ex, p, len(zkey_bytes), rank, world,
                           shard_flags(split, block_log))

    def load_zkey_shard_split(self, zkey_bytes, rank, world):
        """Like load_zkey_shard, with the H-scalar chain split too: this rank's constraint rows (c = rank mod
        world) of the coefficient list and the cyclic H-point shard H[t*world + rank]."""
        p, k = _buf(zkey_bytes)
        return ZKey._adopt(self, lib().zkpoa_zkey_load_shard_split, p, len(zkey_bytes), rank, world)

    def witness_load(self, zkey, wtns_bytes):
        """Parse a .wtns and upload it into the key's witness buffer -> public bytes."""
        pw, kw = _buf(wtns_bytes)
        pub = _Out(32 * zkey.info()[1])
        self._check(lib().zkpoa_witness_load(self._h, zkey._h, pw, len(wtns_bytes), pub, pub.n), "zkpoa_witness_load")
        return pub.bytes()

    def split_stage1(self, zkey, d_witness, d_exchange):
        self._check(lib().zkpoa_split_stage1(self._h, zkey._h, d_witness, d_exchange), "zkpoa_split_stage1")

    def split_stage2(self, zkey, d_received, d_exchange):
        self._check(lib().zkpoa_split_stage2(self._h, zkey._h, d_received, d_exchange), "zkpoa_split_stage2")

    def split_stage3(self, zkey, d_received):
        self._check(lib().zkpoa_split_stage3(self._h, zkey._h, d_received), "zkpoa_split_stage3")

    def prove_partials(self, zkey, wtns_bytes):
        """-> (partials[384] = A|B1|B2|C|H MSM results of the key's shard, public bytes)"""
        pw, kw = _buf(wtns_bytes)
        parts = ctypes.create_string_buffer(384)
        pub = _Out(32 * zkey.info()[1])
        self._check(lib().zkpoa_prove_partials(self._h, zkey._h, pw, len(wtns_bytes), parts, pub, pub.n),
                    "zkpoa_prove_partials")
        return parts.raw, pub.bytes()

    def prove_partials_device(self, zkey, d_witness):
        parts = ctypes.create_string_buffer(384)
        self._check(lib().zkpoa_prove_partials_device(self._h, zkey._h, d_witness, parts), "zkpoa_prove_partials_device")
        return parts.raw

    def read_h_scalars(self, zkey, count):
        """H-MSM scalars of the last prove on `zkey` (count x 32 B standard form) as a numpy uint64 [count, 4]."""
        import numpy as np
        out = np.empty((count, 4), dtype=np.uint64)
        self._check(lib().zkpoa_zkey_read_h_scalars(self._h, zkey._h, out.ctypes.data, out.nbytes),
                    "zkpoa_zkey_read_h_scalars")
        return out

    def prove_device(self, zkey, d_witness, r=None, s=None):
        """Prove with the witness already in HBM -> (proof_points[256], public bytes)."""
        proof = ctypes.create_string_buffer(256)
        pub = _Out(32 * zkey.info()[1])
        self._check(lib().zkpoa_prove_device(self._h, zkey._h, d_witness, _scalar(r), _scalar(s), proof, pub, pub.n),
                    "zkpoa_prove_device")
        return proof.raw, pub.bytes()

    def prove(self, zkey, wtns_bytes, r=None, s=None):
        """-> (proof_points[256 bytes], public[nPublic*32 bytes])"""
        pw, kw = _buf(wtns_bytes)
        proof = ctypes.create_string_buffer(256)
        pub = _Out(32 * zkey.info()[1])
        self._check(lib().zkpoa_prove(self._h, zkey._h, pw, len(wtns_bytes), _scalar(r), _scalar(s), proof, pub, pub.n),
                    "zkpoa_prove")
        return proof.raw, pub.bytes()


class _Handle:
    """A native object that lives inside a Context: `_ctx`, the handle `_h`, and one way to let go of it. A subclass
    states `_free(ctx_handle, handle)`; it runs once, and only while the context is still open (destroying the context
    has freed what hung off it)."""

    def _open(self, ctx, load, *args):
        """load(ctx, *args, &handle), a loader of the C ABI, makes the native object; a failure names the loader."""
        self._ctx, self._h = ctx, ctypes.c_void_p()
        ctx._check(load(ctx._h, *args, ctypes.byref(self._h)), load.__name__)

    def close(self):
        if self._h and self._ctx._h:
            self._free(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MerkleTree(_Handle):
    """The anonymity-set Poseidon Merkle tree resident in HBM (zkpoa_merkle_build)."""

    def __init__(self, ctx, addresses, balances, device=False, n=None):
        if device:
            self._open(ctx, lib().zkpoa_merkle_build_device, addresses, balances, n)
        else:
            n = len(addresses) // 32 if n is None else n
            pa, ka = _buf(addresses)
            pb, kb = _buf(balances)
            self._open(ctx, lib().zkpoa_merkle_build, pa, pb, n)

    def _free(self, ctx_h, h):
        lib().zkpoa_merkle_free(ctx_h, h)

    def info(self):
        """(n, path length, nodes)"""
        out = (ctypes.c_uint64 * 3)()
        lib().zkpoa_merkle_info(self._h, out)
        return tuple(int(v) for v in out)

    def root(self):
        out = ctypes.create_string_buffer(32)
        self._ctx._check(lib().zkpoa_merkle_root(self._ctx._h, self._h, out), "zkpoa_merkle_root")
        return int.from_bytes(out.raw, "little")

    def leaves(self, first=0, count=None):
        count = (1 << self.info()[1]) - first if count is None else count
        out = _Out(32 * count)
        self._ctx._check(lib().zkpoa_merkle_leaves(self._ctx._h, self._h, first, count, out), "zkpoa_merkle_leaves")
        return out.bytes()

    def path(self, index):
        """(sibling hashes from the leaves up as ints, index bits)"""
        k = self.info()[1]
        elems, bits = _Out(32 * k), _Out(k)
        self._ctx._check(lib().zkpoa_merkle_path(self._ctx._h, self._h, index, elems, bits), "zkpoa_merkle_path")
        raw = elems.bytes()
        return ([int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(k)], list(bits.bytes()))

    def find(self, hashes):
        """Leaf hashes (m x 32 B LE) looked up among the set's own leaves (padding is never searched) -> (first, count),
        numpy uint32 arrays: the lowest row that holds the hash (0xFFFFFFFF: none) and how many rows do."""
        import numpy as np
        m = len(hashes) // 32
        p, keep = _buf(hashes)
        first, count = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
        self._ctx._check(lib().zkpoa_merkle_find(self._ctx._h, self._h, p, m, first.ctypes.data, count.ctypes.data),
                         "zkpoa_merkle_find")
        return first, count

    def paths(self, indices):
        """The sibling paths of any number of leaves in one go -> (m x k x 32 B, m x k index bits as bytes): what m calls
        of path() give, back to back."""
        import numpy as np
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        m, k = len(idx), self.info()[1]
        elems, bits = _Out(32 * k * m), _Out(k * m)
        self._ctx._check(lib().zkpoa_merkle_paths(self._ctx._h, self._h, idx.ctypes.data, m, elems, bits), "zkpoa_merkle_paths")
        return elems.bytes(), bits.bytes()

    def paths_device(self, d_indices, m, d_out):
        """The gather kernel alone: d_indices (m x u64) and d_out (m x k x 32 B) are device pointers; an index that is
        not below 2^k gives a path of zeros."""
        self._ctx._check(lib().zkpoa_merkle_paths_device(self._ctx._h, self._h, d_indices, m, d_out), "zkpoa_merkle_paths_device")


class MsmTable(_Handle):
    """Fixed-base table 2^(c*j) * P_i of a resident base array (zkpoa_msm_table_build)."""

    def __init__(self, ctx, group, d_bases, n, window_bits=0):
        self.group = group
        self._open(ctx, lib().zkpoa_msm_table_build, group, d_bases, n, window_bits)

    def _free(self, ctx_h, h):
        lib().zkpoa_msm_table_free(ctx_h, h)

    def info(self):
        """(n, window_bits, windows, bytes)"""
        out = (ctypes.c_uint64 * 4)()
        lib().zkpoa_msm_table_info(self._h, out)
        return tuple(int(v) for v in out)


class ZKey(_Handle):
    """A proving key resident in HBM (zkey sections 4-9 uploaded once)."""

    def __init__(self, ctx, zkey_bytes):
        p, k = _buf(zkey_bytes)
        self._open(ctx, lib().zkpoa_zkey_load, p, len(zkey_bytes))

    @classmethod
    def _adopt(cls, ctx, load, *args):
        """The key that one of the other loaders makes: load(ctx, *args, &key), see _Handle._open."""
        key = cls.__new__(cls)
        key._open(ctx, load, *args)
        return key

    def _free(self, ctx_h, h):
        lib().zkpoa_zkey_free(ctx_h, h)

    def info(self):
        out = (ctypes.c_uint64 * 4)()
        lib().zkpoa_zkey_info(self._h, out)
        return tuple(int(v) for v in out)

    def set_shard(self, rank, world):
        """Restrict a fully resident key to shard `rank` of `world` (for zkpoa_prove_partials)."""
        if lib().zkpoa_zkey_set_shard(self._h, rank, world) != PROVER_OK:
            raise ZkpoaError("zkpoa_zkey_set_shard failed")

    def set_shard_split(self, rank, world):
        """set_shard + the H-scalar chain split over the same ranks (world in 2, 4, 8)."""
        self._ctx._check(lib().zkpoa_zkey_set_shard_split(self._ctx._h, self._h, rank, world),
                         "zkpoa_zkey_set_shard_split")

    def precompute(self, budget_bytes=0):
        """Build the key's fixed-base tables (H, C, A, B while they fit; 0 = half of the free HBM) -> bytes used."""
        used = ctypes.c_uint64(0)
        self._ctx._check(lib().zkpoa_zkey_precompute(self._ctx._h, self._h, budget_bytes, ctypes.byref(used)),
                         "zkpoa_zkey_precompute")
        return int(used.value)

    def vkey_points(self):
        """The verification key the zkey carries (sections 2-3): alpha1(64) beta2(128) gamma2(128) delta2(128) +
        IC[(nPublic+1) x 64], wire format; None for keys assembled from device buffers."""
        rc, (buf,) = _sized(lambda *out: lib().zkpoa_zkey_vkey(self._h, *out), 0)
        if buf is None:         # the question for the size was not answered with one: the handle has no key
            return None
        if rc != PROVER_OK:
            raise ZkpoaError("zkpoa_zkey_vkey failed")
        return buf.raw

    def header(self):
        """alpha1(64) beta1(64) beta2(128) delta1(64) delta2(128), wire format."""
        out = ctypes.create_string_buffer(448)
        lib().zkpoa_zkey_header(self._h, out)
        return out.raw


def _json_call(fn, *args):
    rc, (buf,) = _sized(lambda *out: fn(*args, *out), 0)
    if rc != PROVER_OK:
        raise ZkpoaError("json conversion failed")
    return buf.value.decode()


def proof_to_json(proof_points, style="rapidsnark"):
    p, k = _buf(proof_points)
    return _json_call(lib().zkpoa_proof_to_json, p, 0 if style == "rapidsnark" else 1)


def public_to_json(public_le, style="rapidsnark"):
    p, k = _buf(public_le if len(public_le) else b"\0")
    return _json_call(lib().zkpoa_public_to_json, p, len(public_le) // 32, 0 if style == "rapidsnark" else 1)


def groth16_verify(vkey_json, public_json, proof_json):
    """`snarkjs groth16 verify` on the three JSON texts (host only) -> True / False; raises on malformed input."""
    err = ctypes.create_string_buffer(512)
    rc = lib().zkpoa_groth16_verify(vkey_json.encode(), public_json.encode(), proof_json.encode(), err, 512)
    if rc == PROVER_OK:
        return True
    if rc == 0x10:
        return False
    raise ZkpoaError("zkpoa_groth16_verify: " + err.value.decode())


def eth_block_header(rlp):
    """A block header's RLP -> (its hash, the state root, the number); host only. ZkpoaError for what is no header."""
    h, root, number = _Out(32), _Out(32), ctypes.c_uint64(0)
    if lib().zkpoa_eth_block_header(bytes(rlp) or None, len(rlp), h, root, ctypes.byref(number)) != PROVER_OK:
        raise ZkpoaError("zkpoa_eth_block_header: not the RLP of a block header")
    return h.bytes(), root.bytes(), int(number.value)


def export_vkey(zkey_bytes):
    """`snarkjs zkey export verificationkey`: the text of <circuit>_vkey.json from a zkey image (host only)."""
    p, k = _buf(zkey_bytes)
    err = ctypes.create_string_buffer(512)
    rc, (buf,) = _sized(lambda *out: lib().zkpoa_zkey_export_vkey(p, len(zkey_bytes), *out, err, 512), 0)
    if rc != PROVER_OK:
        raise ZkpoaError("zkpoa_zkey_export_vkey: " + err.value.decode())
    return buf.value.decode()


def poseidon_params():
    """(round constants, MDS rows) the library generates (host only), as Python ints."""
    buf = ctypes.create_string_buffer(204 * 32)
    if lib().zkpoa_poseidon_params(buf) != PROVER_OK:
        raise ZkpoaError("zkpoa_poseidon_params failed")
    vals = [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(204)]
    return vals[:195], [vals[195 + 3 * i:198 + 3 * i] for i in range(3)]


def _le32(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def poseidon_hash(inputs, init_state=0, n_out=1):
    """circomlibjs poseidon(inputs, initState, nOut) for 1..16 inputs (host only) -> the first n_out state elements."""
    out = ctypes.create_string_buffer(32 * max(1, n_out))
    if lib().zkpoa_poseidon_hash(_le32(inputs), len(inputs), _le32([init_state]), n_out, out) != PROVER_OK:
        raise ZkpoaError("zkpoa_poseidon_hash: 1..16 inputs below the field's order and 1..len + 1 outputs are needed")
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n_out)]


def poseidon_sponge(inputs):
    """The reference's poseidonSponge (input_prep_for_layer_two.ts) over one or more field elements; host only."""
    out = ctypes.create_string_buffer(32)
    if lib().zkpoa_poseidon_sponge(_le32(inputs), len(inputs), out) != PROVER_OK:
        raise ZkpoaError("zkpoa_poseidon_sponge: at least one input, all below the field's order, is needed")
    return int.from_bytes(out.raw, "little")


def pedersen_commit(secret, blinding):
    """secret * G + blinding * H on ed25519 as the reference computes it (host only) -> (x, y, z, t)."""
    out = ctypes.create_string_buffer(128)
    if lib().zkpoa_pedersen_commit(_le32([secret]), _le32([blinding]), out) != PROVER_OK:
        raise ZkpoaError("zkpoa_pedersen_commit failed")
    return tuple(int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(4))


def pedersen_check(secret, blinding, signals):
    """Is that commitment the point in the first 12 public signals of the layer-three circuit? Host only."""
    if len(signals) < 12:
        raise ZkpoaError("pedersen_check: the commitment is the first 12 public signals, %d given" % len(signals))
    equal = ctypes.c_int(0)
    if lib().zkpoa_pedersen_check(_le32([secret]), _le32([blinding]), _le32(signals[:12]), ctypes.byref(equal)) != PROVER_OK:
        raise ZkpoaError("zkpoa_pedersen_check failed")
    return bool(equal.value)


def pedersen_decode(signals):
    """The point the layer-three circuit's first 12 public signals spell -> its 32-byte RFC 8032 encoding, or None when
    a signal is 2^85 or more, Z = 0 or the coordinates are not on ed25519. Torsion is not checked. Host only."""
    if len(signals) < 12:
        raise ZkpoaError("pedersen_decode: the commitment is the first 12 public signals, %d given" % len(signals))
    out = ctypes.create_string_buffer(32)
    valid = ctypes.c_int(0)
    if lib().zkpoa_pedersen_decode(_le32(signals[:12]), out, ctypes.byref(valid)) != PROVER_OK:
        raise ZkpoaError("zkpoa_pedersen_decode failed")
    return out.raw if valid.value else None


def groth16_verify_points(vkey_points, proof_points, public_le):
    """The same check on wire-format points (ZKey.vkey_points(), Context.prove() outputs); host only."""
    err = ctypes.create_string_buffer(512)
    pub = bytes(public_le)
    rc = lib().zkpoa_groth16_verify_points(bytes(vkey_points), len(vkey_points), bytes(proof_points),
                                           pub if pub else None, len(pub) // 32, err, 512)
    if rc == PROVER_OK:
        return True
    if rc == 0x10:
        return False
    raise ZkpoaError("zkpoa_groth16_verify_points: " + err.value.decode())


def sanitize_proof(vkey_json, public_json, proof_json):
    """The text sanitize_groth16_proof.py writes to sanitized_proof.json (host only)."""
    err = ctypes.create_string_buffer(512)
    rc, (buf,) = _sized(lambda *out: lib().zkpoa_sanitize_proof(vkey_json.encode(), public_json.encode(),
                                                                proof_json.encode(), *out, err, 512), 1 << 16)
    if rc != PROVER_OK:
        raise ZkpoaError("zkpoa_sanitize_proof: " + err.value.decode())
    return buf.value.decode()


def prove_assemble(header_points, partial_sums, r=None, s=None):
    """Host-only randomised assembly: header (448 B) + summed partials (384 B) + r, s -> proof_points[256]."""
    out = ctypes.create_string_buffer(256)
    if lib().zkpoa_prove_assemble(bytes(header_points), bytes(partial_sums), _scalar(r), _scalar(s), out) != PROVER_OK:
        raise ZkpoaError("zkpoa_prove_assemble failed")
    return out.raw


def sum_partials(partials_list):
    """Component-wise sum of per-rank partials (each 384 B = A|B1|B2|C|H) -> 384 B."""
    g1 = lambda lo: g1_sum(b"".join(p[lo:lo + 64] for p in partials_list))
    b2 = g2_sum(b"".join(p[128:256] for p in partials_list))
    return g1(0) + g1(64) + b2 + g1(256) + g1(320)


def g1_sum(points):
    p, k = _buf(points)
    out = ctypes.create_string_buffer(64)
    lib().zkpoa_g1_sum(p, len(points) // 64, out)
    return out.raw


def g2_sum(points):
    p, k = _buf(points)
    out = ctypes.create_string_buffer(128)
    lib().zkpoa_g2_sum(p, len(points) // 128, out)
    return out.raw


# ---- HD wallets, host only (include/zkpoa_hd_wallet.h) ----------------------------------------------------------------
def bip32_master(seed):
    """The master key of a 16..64 B seed -> (key data 00 || k, chain code)."""
    key, chain = _Out(33), _Out(32)
    if lib().zkpoa_bip32_master(_buf(bytes(seed))[0], len(seed), key, chain) != PROVER_OK:
        raise ZkpoaError("zkpoa_bip32_master: a seed of 16..64 bytes whose key is in [1, group order) is needed")
    return key.bytes(), chain.bytes()


def bip39_seed(mnemonic, passphrase=""):
    """The 64 B seed of a mnemonic (PBKDF2-HMAC-SHA512, 2048 rounds). ASCII only; neither the word list nor the checksum
    is checked."""
    out = _Out(64)
    try:
        args = mnemonic.encode("ascii"), passphrase.encode("ascii")
    except UnicodeEncodeError:
        raise ZkpoaError("bip39_seed: ASCII only (NFKD normalisation is not implemented)")
    if b"\0" in args[0] + args[1] or lib().zkpoa_bip39_seed(args[0], args[1], out) != PROVER_OK:
        raise ZkpoaError("zkpoa_bip39_seed: an ASCII mnemonic and passphrase of at most 4096 bytes each are needed")
    return out.bytes()


def bip32_parse_key(text):
    """An xprv / xpub string -> (key data, chain code, depth, child index); ZkpoaError for anything else."""
    key, chain, where = _Out(33), _Out(32), (ctypes.c_uint32 * 2)()
    if "\0" in text or lib().zkpoa_bip32_parse_key(text.encode("utf-8", "replace"), key, chain, where) != PROVER_OK:
        raise ZkpoaError("zkpoa_bip32_parse_key: not an xprv / xpub (alphabet, length, checksum, version or key)")
    return key.bytes(), chain.bytes(), int(where[0]), int(where[1])


def bip32_parse_path(path):
    """"m/44'/60'/0'/0" -> [indices], a hardened level with bit 31 set; ZkpoaError for anything that is no path."""
    index, levels = (ctypes.c_uint32 * 255)(), ctypes.c_uint32(0)
    if "\0" in path or lib().zkpoa_bip32_parse_path(path.encode("utf-8", "replace"), index, ctypes.byref(levels)) != PROVER_OK:
        raise ZkpoaError("zkpoa_bip32_parse_path: not a path of at most 255 levels: %r" % path)
    return list(index[:levels.value])


def g1_mul(point, k):
    out = ctypes.create_string_buffer(64)
    lib().zkpoa_g1_mul(point, _scalar(k), out)
    return out.raw


def g2_mul(point, k):
    out = ctypes.create_string_buffer(128)
    lib().zkpoa_g2_mul(point, _scalar(k), out)
    return out.raw


def ptau_contributions(ptau_path):
    """Host only: -> (count, ["contribution <name> <response hash>" | "beacon <name> <response hash>", ...]) of a .ptau's
    section 7; ZkpoaError for an unreadable file or a malformed section."""
    cnt = ctypes.c_uint32(0)
    if lib().zkpoa_ptau_contributions(os.fsencode(ptau_path), ctypes.byref(cnt), None, 0):
        raise ZkpoaError("zkpoa_ptau_contributions failed")
    text = ctypes.create_string_buffer(int(cnt.value) * 400 + 1)          # a line is at most 13 + 255 + 1 + 128 + 1 bytes
    if lib().zkpoa_ptau_contributions(os.fsencode(ptau_path), ctypes.byref(cnt), text, len(text)):
        raise ZkpoaError("zkpoa_ptau_contributions failed")
    return int(cnt.value), text.value.decode().splitlines()


def blake2b_state(data):
    """The 216-byte Blake2b-512 state after `data` (a contribution record's partialHash form)."""
    h = lib().zkpoa_blake2b_new()
    lib().zkpoa_blake2b_update(h, bytes(data), len(data))
    out = ctypes.create_string_buffer(216)
    lib().zkpoa_blake2b_state(h, out)
    lib().zkpoa_blake2b_final(h, ctypes.create_string_buffer(64))
    return out.raw


def blake2b_resume(state, data):
    """The digest of a saved state continued with `data`; ZkpoaError for a state that cannot be one."""
    h = lib().zkpoa_blake2b_restore(bytes(state))
    if not h:
        raise ZkpoaError("zkpoa_blake2b_restore: not a Blake2b state")
    lib().zkpoa_blake2b_update(h, bytes(data), len(data))
    out = ctypes.create_string_buffer(64)
    lib().zkpoa_blake2b_final(h, out)
    return out.raw


def zkey_contributions(zkey_path):
    """(the key carries a transcript, [(type, name), ...]) of a .zkey's section 10 (host only)."""
    has, cnt, text = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.create_string_buffer(1 << 16)
    if lib().zkpoa_zkey_contributions(os.fsencode(zkey_path), ctypes.byref(has), ctypes.byref(cnt), text, len(text)):
        raise ZkpoaError("zkpoa_zkey_contributions failed")
    lines = text.value.decode().split("\n")[:cnt.value]
    return bool(has.value), [tuple(l.split(" ", 1)) for l in lines]


# ---- host-only primitives of the phase-2 transcript (csrc/phase2.hpp), for the tests
def blake2b512(data):
    out = ctypes.create_string_buffer(64)
    lib().zkpoa_blake2b512(bytes(data), len(data), out)
    return out.raw


def blake2b512_stream(pieces):
    st, out = lib().zkpoa_blake2b_new(), ctypes.create_string_buffer(64)
    for p in pieces:
        lib().zkpoa_blake2b_update(st, bytes(p), len(p))
    lib().zkpoa_blake2b_final(st, out)
    return out.raw


def sha256(data):
    out = ctypes.create_string_buffer(32)
    lib().zkpoa_sha256(bytes(data), len(data), out)
    return out.raw


def _key(words):
    return (ctypes.c_uint32 * 8)(*words)


class ChaCha:
    """ffjavascript's ChaCha generator (key: eight u32 words)."""

    def __init__(self, key):
        self._h = lib().zkpoa_chacha_new(_key(key))

    def next_u32(self):
        return lib().zkpoa_chacha_next_u32(self._h)

    def next_u64(self):
        return lib().zkpoa_chacha_next_u64(self._h)

    def next_bool(self):
        return bool(lib().zkpoa_chacha_next_bool(self._h))

    def __del__(self):
        if self._h:
            lib().zkpoa_chacha_free(self._h)
            self._h = None


def fq_sqrt(a):
    out = ctypes.create_string_buffer(32)
    return int.from_bytes(out.raw, "little") if lib().zkpoa_fq_sqrt(_scalar(a), out) else None


def fq2_sqrt(a):
    out = ctypes.create_string_buffer(64)
    if not lib().zkpoa_fq2_sqrt(_scalar(a[0]) + _scalar(a[1]), out):
        return None
    return (int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little"))


def fr_from_rng(key):
    out = ctypes.create_string_buffer(32)
    lib().zkpoa_fr_from_rng(_key(key), out)
    return int.from_bytes(out.raw, "little")


def g1_from_rng(key):
    out = ctypes.create_string_buffer(64)
    lib().zkpoa_g1_from_rng(_key(key), out)
    return out.raw


def g2_from_rng(key):
    out = ctypes.create_string_buffer(128)
    lib().zkpoa_g2_from_rng(_key(key), out)
    return out.raw


def hash_to_g2(hash64):
    out = ctypes.create_string_buffer(128)
    lib().zkpoa_hash_to_g2(bytes(hash64), out)
    return out.raw


def beacon_key(beacon, num_iterations_exp):
    key = (ctypes.c_uint32 * 8)()
    if lib().zkpoa_beacon_key(bytes(beacon), len(beacon), num_iterations_exp, key):
        raise ZkpoaError("zkpoa_beacon_key: numIterationsExp above 30")
    return list(key)


def _prove_to_files(what, prover, proof_path, public_path):
    """prover(proof buffer, &size, public buffer, &size, error buffer, its size) is one of the one-shot entry points with
    its inputs bound: the two JSON texts go to their files. The first buffers (4 KiB, 1 MiB) hold any proof the
    reference's circuits make, so the prover runs once; only a short buffer makes it run again."""
    err = ctypes.create_string_buffer(1024)
    rc, (proof, public) = _sized(lambda *out: prover(*out, err, 1024), 1 << 12, 1 << 20)
    if rc != PROVER_OK:
        raise ZkpoaError("%s failed (%d): %s" % (what, rc, err.value.decode()))
    _replace_file(proof_path, proof.value)
    _replace_file(public_path, public.value)


def groth16_prove(zkey_path, wtns_path, proof_path, public_path):
    """The reference's prove step (scripts/g16_prove.sh:248-252) through the C ABI:
    same four arguments as the `prover` executable."""
    with open(wtns_path, "rb") as f:
        wtns = f.read()
    pw, kw = _buf(wtns)
    _prove_to_files("groth16_prover", lambda *out: lib().groth16_prover_zkey_file(os.fsencode(zkey_path), pw, len(wtns), *out),
                    proof_path, public_path)


def groth16_prove_files(zkey_path, wtns_path, proof_path, public_path):
    """The same step with both inputs as paths (zkpoa_groth16_prover_files: what the `prover` executable calls; the
    witness goes from the page cache straight into the upload's pinned buffers, never mapped or copied on the host)."""
    _prove_to_files("zkpoa_groth16_prover_files",
                    lambda *out: lib().zkpoa_groth16_prover_files(os.fsencode(zkey_path), os.fsencode(wtns_path), *out),
                    proof_path, public_path)
