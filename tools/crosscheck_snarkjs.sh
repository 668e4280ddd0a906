#!/usr/bin/env bash
# Cross-check of this prover against snarkjs on a REAL zkey -- for a maintainer on a box that has snarkjs
# (the build container has neither snarkjs nor a real .zkey/.wtns: SURVEY.md 8c; this script was never run there).
#
#   tools/crosscheck_snarkjs.sh <circuit_final.zkey> <witness.wtns> [workdir]
#
# What it does, mirroring the reference's own prove -> verify sequence
# (scripts/g16_prove.sh:246-252, scripts/g16_verify.sh:213-216, scripts/g16_setup.sh:287-293):
#   1. `prover zkey wtns proof.json public.json`               (this repo's drop-in, self-check ON)
#   2. `snarkjs zkey export verificationkey zkey vkey.json`    (the reference's own export), byte-compared with
#      `zkpoa-verify --export-vkey` on the same zkey
#   3. `snarkjs groth16 verify vkey.json public.json proof.json`  -> must print "snarkJS: OK!"
#   4. the native verifier on the same three files            -> must agree
#   5. `snarkjs groth16 prove` on the same inputs; public.json must be byte-identical, and with
#      ZKPOA_JSON=snarkjs our public.json must equal snarkjs' byte for byte. (proof.json differs: r, s are random
#      on both sides; "bit-identical proofs" only exists for injected r, s -- BASELINE north_star)
# Exit code 0 = every step agreed.
#
#   tools/crosscheck_snarkjs.sh --zkey-trail <circuit.r1cs> <pot.ptau> [workdir]
#
# The phase-2 transcript: is a key made HERE accepted by `snarkjs zkey verify`, and one made by
# snarkjs by `zkpoa-setup zkey verify`? The .ptau must be prepared for phase 2 and carry section 2. Never run so far:
#   a. `zkpoa-setup zkey new --transcript`, `zkey contribute --name=...`, `zkey beacon <hex> 10`
#   b. `snarkjs zkey verify r1cs ptau <that key>`            -> must print "ZKey Ok!"
#   c. `snarkjs zkey new`, `zkey contribute`, `zkey beacon` -> `zkpoa-setup zkey verify` on snarkjs' key must exit 0
#   d. both initial keys must carry the same circuit hash (section 10's first 64 bytes: same r1cs, same ptau)
#
#   tools/crosscheck_snarkjs.sh --ptau-trail <power> [workdir]
#
# The phase-1 transcript: is a ceremony file made HERE accepted by `snarkjs powersoftau verify`,
# and one made by snarkjs by `zkpoa-setup powersoftau verify`? Never run so far:
#   a. `zkpoa-setup powersoftau new`, `contribute --name=...`, `beacon <hex> 10`, `prepare phase2`, `verify`
#   b. `snarkjs powersoftau verify <that file>`             -> must print "Powers of Tau Ok!"
#   c. `snarkjs powersoftau new`, `contribute`, `beacon`, `prepare phase2` -> `zkpoa-setup powersoftau verify` must exit 0
#   d. the two fresh files must be the same file (every point the generator, no record)
set -euo pipefail

if [ "${1:-}" = "--ptau-trail" ]; then
  POWER=${2:?usage: crosscheck_snarkjs.sh --ptau-trail <power> [workdir]}
  WORK=${3:-$(mktemp -d)}
  HERE=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
  SETUP="$HERE/zk-proof-of-assets_amd/zkpoa-setup"
  SNARKJS=${SNARKJS:-npx snarkjs}
  BEACON=0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f
  mkdir -p "$WORK"
  echo "== a. a ceremony file made here"
  "$SETUP" powersoftau new bn128 "$POWER" "$WORK/ours_0.ptau"
  "$SETUP" powersoftau contribute "$WORK/ours_0.ptau" "$WORK/ours_1.ptau" --name="First contributor"
  "$SETUP" powersoftau beacon "$WORK/ours_1.ptau" "$WORK/ours_2.ptau" "$BEACON" 10 --name="Final Beacon"
  "$SETUP" powersoftau prepare phase2 "$WORK/ours_2.ptau" "$WORK/ours_final.ptau"
  "$SETUP" powersoftau verify "$WORK/ours_final.ptau"
  echo "== b. snarkjs powersoftau verify on it"
  $SNARKJS powersoftau verify "$WORK/ours_final.ptau" | tee "$WORK/snarkjs_ptau_verify.log"
  grep -q "Powers of Tau Ok!" "$WORK/snarkjs_ptau_verify.log"
  echo "== c. a ceremony file made by snarkjs, verified here"
  $SNARKJS powersoftau new bn128 "$POWER" "$WORK/sj_0.ptau"
  $SNARKJS powersoftau contribute "$WORK/sj_0.ptau" "$WORK/sj_1.ptau" --name="First contributor" -e="random text"
  $SNARKJS powersoftau beacon "$WORK/sj_1.ptau" "$WORK/sj_2.ptau" "$BEACON" 10 -n="Final Beacon"
  $SNARKJS powersoftau prepare phase2 "$WORK/sj_2.ptau" "$WORK/sj_final.ptau"
  "$SETUP" powersoftau verify "$WORK/sj_final.ptau"
  echo "== d. the two fresh files must be the same file"
  cmp "$WORK/ours_0.ptau" "$WORK/sj_0.ptau"
  echo "crosscheck OK: snarkjs accepts our trail, we accept snarkjs' trail, the fresh files are identical"
  echo "(files kept in $WORK)"
  exit 0
fi

if [ "${1:-}" = "--zkey-trail" ]; then
  R1CS=${2:?usage: crosscheck_snarkjs.sh --zkey-trail <circuit.r1cs> <pot.ptau> [workdir]}
  PTAU=${3:?usage: crosscheck_snarkjs.sh --zkey-trail <circuit.r1cs> <pot.ptau> [workdir]}
  WORK=${4:-$(mktemp -d)}
  HERE=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
  SETUP="$HERE/zk-proof-of-assets_amd/zkpoa-setup"
  SNARKJS=${SNARKJS:-npx snarkjs}
  BEACON=0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f
  mkdir -p "$WORK"
  echo "== a. a key with a transcript made here"
  "$SETUP" zkey new "$R1CS" "$PTAU" "$WORK/ours_0.zkey" --transcript
  "$SETUP" zkey contribute "$WORK/ours_0.zkey" "$WORK/ours_1.zkey" --name="First contributor"
  "$SETUP" zkey beacon "$WORK/ours_1.zkey" "$WORK/ours_final.zkey" "$BEACON" 10 -n="Final Beacon"
  "$SETUP" zkey verify "$R1CS" "$PTAU" "$WORK/ours_final.zkey"
  echo "== b. snarkjs zkey verify on it"
  $SNARKJS zkey verify "$R1CS" "$PTAU" "$WORK/ours_final.zkey" | tee "$WORK/snarkjs_verify.log"
  grep -q "ZKey Ok!" "$WORK/snarkjs_verify.log"
  echo "== c. a key made by snarkjs, verified here"
  $SNARKJS zkey new "$R1CS" "$PTAU" "$WORK/sj_0.zkey"
  $SNARKJS zkey contribute "$WORK/sj_0.zkey" "$WORK/sj_1.zkey" --name="First contributor" -e="random text"
  $SNARKJS zkey beacon "$WORK/sj_1.zkey" "$WORK/sj_final.zkey" "$BEACON" 10 -n="Final Beacon"
  "$SETUP" zkey verify "$R1CS" "$PTAU" "$WORK/sj_final.zkey"
  echo "== d. the two initial keys must be the same file (same circuit hash in section 10)"
  cmp "$WORK/ours_0.zkey" "$WORK/sj_0.zkey"
  echo "crosscheck OK: snarkjs accepts our trail, we accept snarkjs' trail, the initial keys are identical"
  echo "(files kept in $WORK)"
  exit 0
fi

ZKEY=${1:?usage: crosscheck_snarkjs.sh <zkey> <wtns> [workdir]}
WTNS=${2:?usage: crosscheck_snarkjs.sh <zkey> <wtns> [workdir]}
WORK=${3:-$(mktemp -d)}
HERE=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
PROVER="$HERE/zk-proof-of-assets_amd/prover"
VERIFY="$HERE/zk-proof-of-assets_amd/zkpoa-verify"
SNARKJS=${SNARKJS:-npx snarkjs}

mkdir -p "$WORK"
echo "== 1. MI355X prover (self-check against the zkey's own vkey is on by default)"
ZKPOA_SELFCHECK=all ZKPOA_VERBOSE=1 "$PROVER" "$ZKEY" "$WTNS" "$WORK/proof.json" "$WORK/public.json"

echo "== 2. snarkjs zkey export verificationkey"
$SNARKJS zkey export verificationkey "$ZKEY" "$WORK/vkey.json"

echo "== 2b. our export of the same key must be byte-identical (zkey sections 2-3 decoded with the same conventions)"
"$VERIFY" --export-vkey "$ZKEY" "$WORK/vkey_ours.json"
cmp "$WORK/vkey.json" "$WORK/vkey_ours.json"

echo "== 3. snarkjs groth16 verify (the reference's acceptance check, g16_verify.sh:213-216)"
$SNARKJS groth16 verify "$WORK/vkey.json" "$WORK/public.json" "$WORK/proof.json" | tee "$WORK/verify.log"
grep -q "OK" "$WORK/verify.log"

echo "== 4. native verifier on the same files"
"$VERIFY" "$WORK/vkey.json" "$WORK/public.json" "$WORK/proof.json"

echo "== 5. snarkjs groth16 prove on the same inputs: public signals must match byte for byte"
$SNARKJS groth16 prove "$ZKEY" "$WTNS" "$WORK/proof_snarkjs.json" "$WORK/public_snarkjs.json"
ZKPOA_JSON=snarkjs "$PROVER" "$ZKEY" "$WTNS" "$WORK/proof_ours_snarkjs_style.json" "$WORK/public_ours_snarkjs_style.json"
cmp "$WORK/public_snarkjs.json" "$WORK/public_ours_snarkjs_style.json"
"$VERIFY" "$WORK/vkey.json" "$WORK/public_snarkjs.json" "$WORK/proof_snarkjs.json"

echo "crosscheck OK: snarkjs accepts our proof, the native verifier accepts snarkjs' proof, public signals identical"
echo "(files kept in $WORK)"
