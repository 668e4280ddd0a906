"""The C ABI of libzkpoa_prover.so as ctypes sees it: one signature per symbol of include/zkpoa_prover.h, applied in one
place (lib()), and the few idioms every wrapper of the package shares. tests/test_abi.py compares the table with the
header's prototypes parameter by parameter, so a signature that drifts from the header fails without a GPU.
"""
import ctypes
import os

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libzkpoa_prover.so")

PROVER_OK = 0
PROVER_ERROR = 1
PROVER_ERROR_SHORT_BUFFER = 2
PROVER_INVALID_WITNESS_LENGTH = 3
PROVER_ERROR_RUNTIME = 4


class ZkpoaError(RuntimeError):
    pass


# The type codes of the tables below. p: a pointer the caller passes as an int (device pointers, handles), None or a
# ctypes buffer; s: a pointer the caller passes as bytes (paths, names, scalars) or a string buffer; T*: a typed pointer
# (p* = the handle a loader writes). "-" = void. ul is `unsigned long`, l is `long`, u is `unsigned`.
_T = {"-": None, "i": ctypes.c_int, "u": ctypes.c_uint, "u32": ctypes.c_uint32, "u64": ctypes.c_uint64,
      "ul": ctypes.c_ulong, "l": ctypes.c_long, "f": ctypes.c_float, "p": ctypes.c_void_p, "s": ctypes.c_char_p}
_T.update({k + "*": ctypes.POINTER(t) for k, t in list(_T.items()) if t is not None and k != "s"})
_T["d*"] = ctypes.POINTER(ctypes.c_double)

# every symbol include/zkpoa_prover.h declares, in its order: "return type: parameter types"
SIGNATURES = {
    "groth16_prover":                  "i: p ul p ul p ul* p ul* p ul",
    "groth16_prover_zkey_file":        "i: s p ul p ul* p ul* p ul",
    "zkpoa_groth16_prover_files":      "i: s s p ul* p ul* p ul",
    "zkpoa_set_thread_options":        "i: s s s i",
    "zkpoa_clear_thread_options":      "i:",
    "zkpoa_idle_work":                 "i:",
    "zkpoa_context_create":            "i: i p* s ul",
    "zkpoa_context_destroy":           "-: p",
    "zkpoa_last_error":                "s: p",
    "zkpoa_zkey_load":                 "i: p p ul p*",
    "zkpoa_zkey_free":                 "-: p p",
    "zkpoa_zkey_info":                 "i: p u64*",
    "zkpoa_prove":                     "i: p p p ul s s p p ul",
    "zkpoa_zkey_load_device":          "i: p u64 u64 u p p p p p p u64 s p*",
    "zkpoa_zkey_load_device_shard":    "i: p u64 u64 u u64 u64 i p p p p p p u64 s p*",
    "zkpoa_prove_device":              "i: p p p s s p p ul",
    "zkpoa_zkey_load_shard":           "i: p p ul u64 u64 p*",
    "zkpoa_zkey_load_shard_ex":        "i: p p ul u64 u64 i p*",
    "zkpoa_zkey_set_shard":            "i: p u64 u64",
    "zkpoa_zkey_header":               "i: p p",
    "zkpoa_prove_partials":            "i: p p p ul p p ul",
    "zkpoa_prove_partials_device":     "i: p p p p",
    "zkpoa_prove_assemble":            "i: s s s s p",
    "zkpoa_context_stream":            "p: p i",
    "zkpoa_context_synchronize":       "i: p",
    "zkpoa_zkey_load_shard_split":     "i: p p ul u64 u64 p*",
    "zkpoa_zkey_set_shard_split":      "i: p p u64 u64",
    "zkpoa_witness_load":              "i: p p p ul p ul",
    "zkpoa_split_stage1":              "i: p p p p",
    "zkpoa_split_stage2":              "i: p p p p",
    "zkpoa_split_stage3":              "i: p p p",
    "zkpoa_zkey_precompute":           "i: p p u64 u64*",
    "zkpoa_zkey_read_h_scalars":       "i: p p p ul",
    "zkpoa_proof_to_json":             "i: p i p ul*",
    "zkpoa_public_to_json":            "i: p ul i p ul*",
    "zkpoa_msm_g1":                    "i: p p p u64 p",
    "zkpoa_msm_g2":                    "i: p p p u64 p",
    "zkpoa_ntt":                       "i: p p u i",
    "zkpoa_h_scalars":                 "i: p p ul p u64 u p",
    "zkpoa_msm_g1_device":             "i: p p p u64 p",
    "zkpoa_msm_g2_device":             "i: p p p u64 p",
    "zkpoa_ntt_device":                "i: p p u i",
    "zkpoa_msm_g1_device_lane":        "i: p i p p u64 p",
    "zkpoa_last_ms_lane":              "f: p i i",
    "zkpoa_msm_table_build":           "i: p i p u64 i p*",
    "zkpoa_msm_table_free":            "-: p p",
    "zkpoa_msm_table_info":            "i: p u64*",
    "zkpoa_msm_table_run_lane":        "i: p i p p p",
    "zkpoa_gen_bases_g1_device":       "i: p s s u64 u64 p",
    "zkpoa_gen_bases_g2_device":       "i: p s s u64 u64 p",
    "zkpoa_g1_sum":                    "i: p u64 p",
    "zkpoa_g2_sum":                    "i: p u64 p",
    "zkpoa_g1_mul":                    "i: s s p",
    "zkpoa_g2_mul":                    "i: s s p",
    "zkpoa_setup_accumulate":          "i: p i p u64 p p p u64 u64 p",
    "zkpoa_zkey_new":                  "i: p s s s",
    "zkpoa_zkey_new_ex":               "i: p s s s u32",
    "zkpoa_zkey_contribute_ex":        "i: p s s s s",
    "zkpoa_zkey_beacon":               "i: p s s s ul u32 s",
    "zkpoa_zkey_contributions":        "i: s i* u32* s ul",
    "zkpoa_hash_form":                 "i: p i s u64 u64 p s",
    "zkpoa_h_diff":                    "i: p s u64 s",
    "zkpoa_blake2b512":                "i: s ul s",
    "zkpoa_blake2b_new":               "p:",
    "zkpoa_blake2b_update":            "i: p s ul",
    "zkpoa_blake2b_final":             "i: p s",
    "zkpoa_sha256":                    "i: s ul s",
    "zkpoa_chacha_new":                "p: u32*",
    "zkpoa_chacha_next_u32":           "u32: p",
    "zkpoa_chacha_next_u64":           "u64: p",
    "zkpoa_chacha_next_bool":          "i: p",
    "zkpoa_chacha_free":               "-: p",
    "zkpoa_fq_sqrt":                   "i: s s",
    "zkpoa_fq2_sqrt":                  "i: s s",
    "zkpoa_fr_from_rng":               "i: u32* s",
    "zkpoa_g1_from_rng":               "i: u32* s",
    "zkpoa_g2_from_rng":               "i: u32* s",
    "zkpoa_hash_to_g2":                "i: s s",
    "zkpoa_beacon_key":                "i: s ul u32 u32*",
    "zkpoa_setup_defer_host_frees":    "-: i",
    "zkpoa_zkey_contribute":           "i: p s s s",
    "zkpoa_wtns_check":                "i: p s s u64* u64*",
    "zkpoa_zkey_verify":               "i: p s s s u32*",
    "zkpoa_ptau_verify":               "i: p s u64 u32* u32*",
    "zkpoa_ec_intt_device":            "i: p i p u32 p",
    "zkpoa_ptau_prepare_phase2":       "i: p s s u32*",
    "zkpoa_scalar_mul_each_device":    "i: p i p p u64 p",
    "zkpoa_power_scalars_device":      "i: p s s u64 u64 p",
    "zkpoa_compressed_form":           "i: p i s u64 u64 p s",
    "zkpoa_ptau_new":                  "i: p u32 s",
    "zkpoa_ptau_contribute":           "i: p s s s s",
    "zkpoa_ptau_beacon":               "i: p s s s ul u32 s",
    "zkpoa_sqrt_device":               "i: p i s u64 p p",
    "zkpoa_decompressed_form":         "i: p i s u64 u64 p",
    "zkpoa_from_hash_form":            "i: p i s u64 u64 p",
    "zkpoa_ptau_export_challenge":     "i: p s s s",
    "zkpoa_ptau_challenge_contribute": "i: p s s s s",
    "zkpoa_ptau_import_response":      "i: p s s s s",
    "zkpoa_ptau_contributions":        "i: s u32* s ul",
    "zkpoa_blake2b_state":             "i: p s",
    "zkpoa_blake2b_restore":           "p: s",
    "zkpoa_groth16_verify":            "i: s s s p ul",
    "zkpoa_sanitize_proof":            "i: s s s p ul* p ul",
    "zkpoa_groth16_verify_points":     "i: p ul p p ul p ul",
    "zkpoa_zkey_vkey":                 "i: p p ul*",
    "zkpoa_zkey_export_vkey":          "i: p ul p ul* p ul",
    "zkpoa_poseidon_params":           "i: p",
    "zkpoa_poseidon2":                 "i: p p p u64 p",
    "zkpoa_poseidon2_device":          "i: p p p u64 p",
    "zkpoa_merkle_build":              "i: p p p u64 p*",
    "zkpoa_merkle_build_device":       "i: p p p u64 p*",
    "zkpoa_merkle_free":               "-: p p",
    "zkpoa_merkle_info":               "i: p u64*",
    "zkpoa_merkle_root":               "i: p p p",
    "zkpoa_merkle_leaves":             "i: p p u64 u64 p",
    "zkpoa_merkle_path":               "i: p p u64 p p",
    "zkpoa_ecdsa_star":                "i: p u64 p p p p p p p p p",
    "zkpoa_keccak256":                 "i: p p u64 u64 p",
    "zkpoa_eth_address":               "i: p p u64 p p",
    "zkpoa_last_ms":                   "f: p i",
    "zkpoa_set_option":                "i: p s l",
    "zkpoa_msm_points_limit":          "u64: p",
    "zkpoa_field_op":                  "i: p i i p p p u64",
    "zkpoa_group_add":                 "i: p i p p p u64",
    "zkpoa_field_prim":                "i: p i i p p u64 i",
    "zkpoa_curve_prim":                "i: p i i p p p p u64",
    "zkpoa_fq29_prim":                 "i: p i p p u64 i",
    "zkpoa_ntt_form":                  "i: p p u i i u u64",
    "zkpoa_test_ntt_plan":             "i: u u u32* u",
    "zkpoa_test_msm_plan":             "i: u64 i i i d* i u64* u",
    "zkpoa_test_msm_sort":             "i: p i p u64 i i i d* i u64* u32* p* u64*",
    "zkpoa_test_msm_density":          "i: p p u64 d*",
}
EXPORTS = list(SIGNATURES)

# every symbol include/zkpoa_layer_inputs.h declares (the header zkpoa_prover.h includes): host only, no context
LAYER_INPUT_SIGNATURES = {
    "zkpoa_poseidon_hash":             "i: s u s u p",
    "zkpoa_poseidon_sponge":           "i: s u64 p",
    "zkpoa_pedersen_commit":           "i: s s p",
    "zkpoa_pedersen_check":            "i: s s s i*",
}

# every symbol include/zkpoa_ecdsa_sign.h declares (zkpoa_prover.h includes that header too): signing, on the GPU
SIGN_SIGNATURES = {
    "zkpoa_sha256_batch":              "i: p p u64 u64 p",
    "zkpoa_secp256k1_pubkey":          "i: p u64 p p p p",
    "zkpoa_secp256k1_derive_keys":     "i: p p u64 u64 u64 p",
    "zkpoa_rfc6979_nonce":             "i: p u64 p p u32 p",
    "zkpoa_ecdsa_sign":                "i: p u64 p p u64 p p p p p p",
}

# every symbol include/zkpoa_hd_wallet.h declares (zkpoa_prover.h includes that header too): BIP-32 key sources; the
# first four and the last on the GPU, the others host only and without a context
HD_SIGNATURES = {
    "zkpoa_sha512_batch":              "i: p p u64 u64 p",
    "zkpoa_hmac_sha512_batch":         "i: p p u64 p u64 u64 p",
    "zkpoa_bip32_children":            "i: p p p u64 u64 p p p p p",
    "zkpoa_bip32_tweak":               "i: p p u64 p p p p p",
    "zkpoa_bip32_master":              "i: p u64 p p",
    "zkpoa_bip39_seed":                "i: s s p",
    "zkpoa_bip32_parse_key":           "i: s p p u32*",
    "zkpoa_bip32_parse_path":          "i: s u32* u32*",
    "zkpoa_bip32_derive_path":         "i: p p p s p p",
}

# every symbol include/zkpoa_audit.h declares (zkpoa_prover.h includes that header too): the verifier's side; the
# third is host only and without a context, the others run on the GPU
AUDIT_SIGNATURES = {
    "zkpoa_anon_set_index_device":     "i: p p u64 p",
    "zkpoa_anon_set_audit":            "i: p p u64 u64*",
    "zkpoa_pedersen_decode":           "i: s p i*",
    "zkpoa_assets_verify":             "i: p p p u64 s s s p u32* p",
}

# every symbol include/zkpoa_merkle_paths.h declares (zkpoa_prover.h includes that header too): the owned leaves at the
# prover's scale, all on the GPU
MERKLE_PATHS_SIGNATURES = {
    "zkpoa_anon_set_find_device":      "i: p p u64 p p u64 p p",
    "zkpoa_merkle_find":               "i: p p p u64 p p",
    "zkpoa_merkle_paths":              "i: p p p u64 p p",
    "zkpoa_merkle_paths_device":       "i: p p p u64 p",
}

# every symbol include/zkpoa_state_proof.h declares (zkpoa_prover.h includes that header too): the set against an
# Ethereum state root; the third is host only and without a context, the others run on the GPU
STATE_PROOF_SIGNATURES = {
    "zkpoa_mpt_verify":                "i: p u64 p i p p u64 u64* u32* u64* p u32* u64*",
    "zkpoa_eth_account_proofs":        "i: p u64 p p p u64 u64* u32* u64* p u32* u64* p p p",
    "zkpoa_eth_block_header":          "i: p u64 p p u64*",
    "zkpoa_anon_set_state_check_file": "i: p p p u64 s p u64 p",
}

# the one symbol include/zkpoa_secp_prim.h declares (zkpoa_prover.h includes that header beside its other test hooks)
SECP_PRIM_SIGNATURES = {
    "zkpoa_secp_prim":                 "i: p i p p u64",
}

# test and measurement hooks the library exports but the public header deliberately leaves out
HOOK_SIGNATURES = {
    "zkpoa_test_upload":               "i: p s u64 u64 p f*",       # csrc/zkpoa_api.hip
    "zkpoa_test_auto_pick_devices":    "i: i u u ul u i*",          # csrc/prover.hip
    "zkpoa_test_multi_block_log":      "u: u64 u",                  # csrc/prover.hip
}


def signature(spec):
    """A table entry as ctypes types: -> (restype, argtypes)."""
    ret, _, params = spec.partition(":")
    return _T[ret], [_T[t] for t in params.split()]


_lib = None


def lib():
    """The loaded shared library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZkpoaError("libzkpoa_prover.so not built (%s): run `python -c 'import __graft_entry__ as g; "
                             "g.build()'` -- there is no CPU fallback" % LIB_PATH)
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64. If our library (linked
        # against /opt/rocm) is loaded first, torch's HSA copy later fails to open the device ("No HIP GPUs
        # are available"); loaded in this order both HIP runtimes share torch's HSA runtime (same SONAME).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for table in (SIGNATURES, LAYER_INPUT_SIGNATURES, SIGN_SIGNATURES, HD_SIGNATURES, AUDIT_SIGNATURES,
                      MERKLE_PATHS_SIGNATURES, STATE_PROOF_SIGNATURES, SECP_PRIM_SIGNATURES, HOOK_SIGNATURES):
            for name, spec in table.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = signature(spec)
        _lib = L
    return _lib


def _buf(b):
    """read-only bytes-like -> (ctypes pointer, keepalive); no copy (a 2^20 MSM hands over 96 MiB per call)."""
    if isinstance(b, bytes):
        return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p), b
    if isinstance(b, bytearray):
        arr = (ctypes.c_char * len(b)).from_buffer(b)
        return ctypes.cast(arr, ctypes.c_void_p), arr
    # numpy array or anything exposing the buffer protocol
    mv = memoryview(b)
    if mv.readonly:
        raw = mv.tobytes()
        return ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p), raw
    arr = (ctypes.c_char * mv.nbytes).from_buffer(b)
    return ctypes.cast(arr, ctypes.c_void_p), arr


class _Out:
    """An n-byte output buffer for a C call, n = 0 included: one byte is allocated then, so that the call still gets
    a pointer; bytes() is the n bytes the call wrote."""

    def __init__(self, n):
        self.n = n
        self._as_parameter_ = ctypes.create_string_buffer(max(1, n))

    def bytes(self):
        return self._as_parameter_.raw[:self.n]


def _scalar(x):
    """An optional 32-byte little-endian scalar: None stays NULL (the library then draws its own)."""
    return None if x is None else int(x).to_bytes(32, "little")


def _name(s):
    """An optional name as the C side takes it."""
    return None if s is None else s.encode()


def _sized(call, *first):
    """The ABI's size protocol ("in: capacity, out: bytes needed"): call(buffer, &size, ...) with one buffer and size
    per entry of `first`, holding that many bytes (0 = a NULL buffer, which only asks for the size); when the answer is
    PROVER_ERROR_SHORT_BUFFER, once more with buffers of the sizes it asked for. -> (the last return code, the buffers
    of that call), so a first guess that fits costs one call."""
    sizes = [ctypes.c_ulong(n) for n in first]

    def attempt():
        bufs = [ctypes.create_string_buffer(s.value) if s.value else None for s in sizes]
        return call(*[x for b, s in zip(bufs, sizes) for x in (b, ctypes.byref(s))]), bufs
    rc, bufs = attempt()
    if rc == PROVER_ERROR_SHORT_BUFFER:
        rc, bufs = attempt()
    return rc, bufs


def _replace_file(path, data):
    """Write under a temporary name, then rename: a reader never sees half a file."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)
