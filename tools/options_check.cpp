// Host check of csrc/options.hpp: the header's own text, compiled by g++ alone (no HIP).
// Build: g++ -O2 -std=c++17 -pthread -I zk-proof-of-assets_amd/csrc tools/options_check.cpp -o options_check
// Use:   options_check OP      in the environment under test (tests/test_options_host.py drives it)
// Sanitizer builds of the same program (no GPU, never on a GPU machine):
//   OPTIONS_CHECK_FLAGS="-O1 -g -fsanitize=address,undefined" python -m pytest tests/test_options_host.py
//   OPTIONS_CHECK_FLAGS="-O1 -g -fsanitize=thread" python -m pytest tests/test_options_host.py -k overlay
//   list            one line per row of the table, tab-separated: name, kind, lo, hi, words, default, strict | lenient,
//                   every | latched, knob | hook, the row's own message or -, meaning
//   get             one line per row: name, tab, what the row's typed accessor returns ("null" or "=<text>" for a text
//                   row), or "error: <message>" where it throws
//   get-twice V     reads every flag / int / choice row, sets every variable to V, and prints a second `get`
//   device LO HI    opt_long(O_DEVICE, LO, HI): the value, or "error: <message>"
//   vlog            one vlog line ("check 7")
//   overlay         two threads, the first with the overlay r = "7", s, json and verbose empty; what each reads of the
//                   four request rows and of ZKPOA_KEY_CACHE: the second thread while the overlay is active, a SideTask
//                   of the first, the first itself, and the first again after it has cleared the overlay
#include "host_threads.hpp"
#include "options.hpp"

#include <future>
#include <iostream>

using namespace zkpoa;

static std::string typed(Opt id) {
  try {
    switch (opt_row(id).kind) {
      case kOptFlag: return opt_flag(id) ? "1" : "0";
      case kOptInt: return std::to_string(opt_long(id));
      case kOptChoice: return std::to_string(opt_choice(id));
      default: break;
    }
    const char* e = opt_text(id);
    return e ? "=" + std::string(e) : "null";
  } catch (const OptionError& e) {
    return std::string("error: ") + e.what();
  }
}

static void get_all() {
  for (int i = 0; i < kOptCount; i++) std::cout << opt_row((Opt)i).name << "\t" << typed((Opt)i) << "\n";
}

static std::string request_rows(const char* who) {
  std::string s = who;
  for (Opt id : {O_R, O_S, O_JSON, O_VERBOSE, O_KEY_CACHE}) s += std::string(" ") + (opt_row(id).name + 6) + " " + typed(id);
  return s + "\n";
}

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "list") {
    static const char* const kinds[] = {"flag", "int", "choice", "text"};
    for (int i = 0; i < kOptCount; i++) {
      const OptRow& r = opt_row((Opt)i);
      std::cout << r.name << "\t" << kinds[r.kind] << "\t" << r.lo << "\t" << r.hi << "\t" << (r.words ? r.words : "-") << "\t"
                << r.dflt << "\t" << (r.bad == kStrict ? "strict" : "lenient") << "\t" << (r.when == kLatched ? "latched" : "every")
                << "\t" << (r.use == kHook ? "hook" : "knob") << "\t" << (r.bad_fmt ? r.bad_fmt : "-") << "\t" << r.meaning << "\n";
    }
  } else if (op == "get") {
    get_all();
  } else if (op == "get-twice" && argc == 3) {
    for (int i = 0; i < kOptCount; i++) (void)typed((Opt)i);
    for (int i = 0; i < kOptCount; i++) setenv(opt_row((Opt)i).name, argv[2], 1);
    get_all();
  } else if (op == "device" && argc == 4) {
    try {
      std::cout << opt_long(O_DEVICE, atol(argv[2]), atol(argv[3])) << "\n";
    } catch (const OptionError& e) {
      std::cout << "error: " << e.what() << "\n";
    }
  } else if (op == "vlog") {
    vlog("check %d\n", 7);
  } else if (op == "overlay") {
    std::promise<void> active, second_done;
    std::string first, second;
    SideTask a([&] {
      OptOverlay& o = opt_overlay();
      o.active = true;
      o.r = "7";
      active.set_value();
      second_done.get_future().wait();
      std::string task;
      SideTask([&] { task = request_rows("task"); }).get();
      first = task + request_rows("first");
      opt_overlay() = OptOverlay();
      first += request_rows("cleared");
    });
    SideTask b([&] {
      active.get_future().wait();
      second = request_rows("second");
      second_done.set_value();
    });
    a.get();
    b.get();
    std::cout << second << first;
  } else {
    std::cerr << "usage: options_check list | get | get-twice V | device LO HI | vlog | overlay\n";
    return 2;
  }
  return 0;
}
