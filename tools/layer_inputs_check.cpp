// Host check of csrc/layer_inputs.hpp (with poseidon_host.hpp and pedersen_host.hpp): the three modes of
// `ecdsa-sigs-parser` compiled by g++ alone, without HIP and without the library.
// Build: g++ -O2 -std=c++17 -pthread -I zk-proof-of-assets_amd/csrc tools/layer_inputs_check.cpp -o layer_inputs_check
// Use:   layer_inputs_check two <parsed> <merkle_root> <merkle_proofs> <hash out> <layer-one proof> <out> <start> <end>
//        layer_inputs_check three <merkle_root> <proof,proof,...> <out> <blinding factor>
//        layer_inputs_check pedersen <parsed> <public.json> <blinding factor>
// Exit status as the command's: 0, or 1 with "Error: ..." on stderr. tests/test_layer_inputs.py drives it on the
// reference's fixtures; LAYER_INPUTS_CHECK_FLAGS adds compiler flags there, which is how the sanitizer build of the same
// program runs (no GPU, never on a GPU machine):
//   LAYER_INPUTS_CHECK_FLAGS="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined" \
//       python -m pytest tests/test_layer_inputs.py -k compiled_alone
#include "layer_inputs.hpp"

using namespace zkpoa::layer_inputs;

int main(int argc, char** argv) {
  try {
    const std::string op = argc > 1 ? argv[1] : "";
    if (op == "two" && argc == 10) {
      LayerTwoPaths p;
      p.input = argv[2];
      p.merkle_root = argv[3];
      p.merkle_proofs = argv[4];
      p.hash_out = argv[5];
      p.layer_one_proof = argv[6];
      p.out = argv[7];
      BatchRange range;
      range.start = atoll(argv[8]);
      range.end = atoll(argv[9]);
      return layer_two_mode(p, range);
    }
    if (op == "three" && argc == 6) return layer_three_mode(argv[2], argv[3], argv[4], argv[5]);
    if (op == "pedersen" && argc == 5) return pedersen_check_mode(argv[2], argv[3], argv[4]);
    fprintf(stderr, "usage: layer_inputs_check two | three | pedersen ...\n");
    return 2;
  } catch (const std::exception& e) {
    fprintf(stderr, "Error: %s\n", e.what());
    return 1;
  }
}
