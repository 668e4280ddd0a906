"""zk-proof-of-assets_amd/csrc/secp256k1.hip.h function by function on the CPU: tools/secp_prim_check.cpp includes the
header's own text, hipcc compiles it for the host alone with AddressSanitizer and UndefinedBehaviorSanitizer, and every
answer -- the operand sets of tests/secp_limb_ref.py through every Fp and Sc function and the recoding, the ladder cases
through fixed_mul, double_mul and recover_one -- is compared with big integers. A stand-alone program: nothing is loaded
into Python, and no GPU is involved. Any sanitizer report ends the program with a non-zero status."""
import os
import shutil
import subprocess

import pytest

import secp_limb_ref as lr
import secp_ref as sr
import sign_ref as sg
from conftest import ROOT

h32 = lambda v: "%064x" % v
HEADER_DIR = os.path.join(ROOT, "zk-proof-of-assets_amd", "csrc")


def build_lines():
    """-> [(kind, name, input line, what to compare the answer with)]"""
    out = []
    for name, cases in lr.prim_sets().items():
        op, _, n8, _ = lr.OPS[name]
        for operands, results in cases:
            want = " ".join([h32(v) for v in results[:n8]] + ["%08x" % v for v in results[n8:]])
            out.append((name, operands, " ".join([str(op)] + [h32(v) for v in operands]), want))
    for k in sg.edge_keys():
        out.append(("fixed_mul", k, "19 " + h32(k), sr.mul(k, sr.G)))
    for name, pt, u2, u1, want in lr.ladder_cases():
        out.append(("double_mul", name, " ".join(["20", h32(pt[0]), h32(pt[1]), h32(u2), h32(u1)]), want))
    for k in (1, 2, 9, lr.N - 1):   # to_affine of a point that is not in its simplest form: (x t^2, y t^3, t^2, t^3)
        x, y = sr.mul(k, sr.G)
        t = 3 + k % 7
        out.append(("to_affine", k, " ".join(["18", h32(x * t * t % lr.P), h32(y * t**3 % lr.P), h32(t * t), h32(t**3)]), h32(x) + " " + h32(y)))
    for name, (r, s, v, z, addr), exp in lr.steered_recoveries():
        want = "%d %s %s %s %s" % (exp[0], h32(exp[1]), h32(exp[2][0]), h32(exp[2][1]), exp[3].hex())
        out.append(("recover", name, "recover %s %s %s %d %s" % (h32(r), h32(s), h32(z), v, addr.hex()), want))
    return out


LINES = build_lines()


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """One build and one run: the answer line of every entry of LINES."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc to compile the host check with")
    exe = str(tmp_path_factory.mktemp("secp_prim_host") / "secp_prim_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O0", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", HEADER_DIR,
                           os.path.join(ROOT, "tools", "secp_prim_check.cpp"), "-o", exe])
    run = subprocess.run([exe], input="\n".join(l[2] for l in LINES) + "\n", capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == ""
    out = run.stdout.splitlines()
    assert len(out) == len(LINES)
    return out


def wrong(answers, kinds, same=lambda got, want: got == want):
    return [(kind, name) for (kind, name, _, want), got in zip(LINES, answers) if kind in kinds and not same(got, want)][:10]


def count(kinds):
    return sum(l[0] in kinds for l in LINES)


def test_fp_products(answers):
    assert count(("fp_mul", "fp_sqr")) >= len(lr.FP_SCALARS) ** 2 + 2000 + len(lr.FP_SCALARS)
    assert wrong(answers, ("fp_mul", "fp_sqr")) == []


def test_fp_sums_and_differences(answers):
    assert wrong(answers, ("fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_ge_p")) == []


def test_fp_power_chains(answers):
    assert count(("fp_inv", "fp_sqrt_candidate")) >= 2 * len(lr.FP_SCALARS)
    assert wrong(answers, ("fp_inv", "fp_sqrt_candidate")) == []


def test_sc_products(answers):
    assert count(("sc_mul",)) >= len(lr.SC_SCALARS) ** 2 + 2000
    assert wrong(answers, ("sc_mul", "sc_inv")) == []


def test_sc_sums_and_comparisons(answers):
    assert wrong(answers, ("sc_add", "sc_neg", "sc_reduce_once", "sc_key_from_hash", "sc_ge_n", "sc_is_high")) == []


def test_recoding(answers):
    assert count(("recode_signed4",)) == len(lr.recode_set())
    canonical = lambda got: "%064x %08x %08x" % lr.recode_canonical(*(int(w, 16) for w in got.split()))
    assert wrong(answers, ("recode_signed4",), lambda got, want: canonical(got) == want) == []


def as_point(line, with_flag):
    """an XYZZ answer as an affine point or None; the is_inf word must say what ZZ says"""
    words = line.split()
    pt = lr.affine_of(*(int(w, 16) for w in words[:4]))
    if with_flag:
        assert int(words[4], 16) == int(pt is None), line
    return pt


def test_fixed_mul_and_to_affine(answers):
    assert count(("fixed_mul",)) == len(sg.edge_keys()) == 21
    assert wrong(answers, ("fixed_mul",), lambda got, want: as_point(got, False) == want) == []
    assert wrong(answers, ("to_affine",)) == []


def test_double_mul(answers):
    assert count(("double_mul",)) == 8 * 11 * 11 + 13
    assert wrong(answers, ("double_mul",), lambda got, want: as_point(got, True) == want) == []


def test_steered_recoveries(answers):
    """recover_one with chosen inner scalars: every output and the status"""
    statuses = [l[3].split()[0] for l in LINES if l[0] == "recover"]
    assert statuses.count("0") >= 60 and {"2", "3", "5"} <= set(statuses)
    assert wrong(answers, ("recover",)) == []
