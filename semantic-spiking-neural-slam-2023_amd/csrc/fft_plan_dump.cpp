// fft_plan_dump.cpp - the planner of ssn_fft_plan.hpp on a CPU, as text (tests/test_fft_plan.py).  Not part of the library:
//   c++ -std=c++17 -O2 fft_plan_dump.cpp -o fft_plan_dump
//   fft_plan_dump routes LENGTH...        LENGTH a number or lo-hi; per length one line for each of the routes
//       stockham-inplace | stockham-outofplace | fourstep-real | fourstep-complex:
//       <route> d <d> L <L> M <M> inplace <0|1> split <N1>x<N2> threads <t> lds <bytes> radices <r>...      (L 0: no route)
//   fft_plan_dump tables <route> LENGTH   that line, then the route's tables, one per line, the floats' bytes in hex:
//       twiddles | chirp | spectrum | g1 | g2
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ssn_fft_plan.hpp"
namespace fft = ssn::fft;

static const char* const ROUTES[] = {"stockham-inplace", "stockham-outofplace", "fourstep-real", "fourstep-complex"};

static fft::Route plan(int which, int d) { return which < 2 ? fft::plan_stockham(d, which == 0) : fft::plan_four_step(d, which == 3); }

static void print_route(int which, int d, const fft::Route& r) {
  std::printf("%s d %d L %d M %d inplace %d split %dx%d threads %d lds %zu radices", ROUTES[which], d, r.L, r.M, r.inplace, r.N1, r.N2,
              r ? fft::threads(r) : 0, r ? fft::lds_bytes(r) : (size_t)0);
  for (int q : r.radix) std::printf(" %d", q);
  std::printf("\n");
}
template <typename P>
static void print_table(const char* name, const std::vector<P>& t) {
  std::printf("%s ", name);
  for (size_t i = 0; i < t.size() * sizeof(P); ++i) std::printf("%02x", ((const unsigned char*)t.data())[i]);
  std::printf("\n");
}
static int usage() {
  std::fprintf(stderr, "usage: fft_plan_dump routes LENGTH|LO-HI ...\n       fft_plan_dump tables ROUTE LENGTH\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "routes")) {
    for (int i = 2; i < argc; ++i) {
      char* end = nullptr;
      const long lo = std::strtol(argv[i], &end, 10);
      const long hi = *end == '-' ? std::strtol(end + 1, &end, 10) : lo;
      if (*end || lo < 1 || hi < lo || hi > 1000000) return usage();
      for (int d = (int)lo; d <= (int)hi; ++d)
        for (int which = 0; which < 4; ++which) print_route(which, d, plan(which, d));
    }
    return 0;
  }
  int which = 0;
  while (which < 4 && (argc != 4 || std::strcmp(argv[2], ROUTES[which]))) ++which;
  const int d = argc == 4 ? std::atoi(argv[3]) : 0;
  if (argc != 4 || std::strcmp(argv[1], "tables") || which == 4 || d < 1) return usage();
  const fft::Route r = plan(which, d);
  print_route(which, d, r);
  if (!r) return 0;
  print_table("twiddles", fft::twiddles(r.L));
  if (r.M > 0) {
    print_table("chirp", fft::chirp(d));
    print_table("spectrum", fft::chirp_spectrum(d, r.M, r.inplace ? &r.radix : nullptr));
  }
  if (r.N1 > 0) {
    print_table("g1", fft::dft4_matrix(r.N1));
    print_table("g2", fft::dft4_matrix(r.N2));
  }
  return 0;
}
