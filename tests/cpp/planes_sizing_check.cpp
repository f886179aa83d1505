// Host-only check of boom_amd/csrc/planes_sizing.h: over a grid of (chains, n, p) the planes
// workspace of the column service covers both of its users --
//   launch_rows_times_columns(R = chains):       planes(n) * chains * p doubles
//   launch_xtwx_cols(R <= column_request_batch): planes(n) * min(batch, R) * p doubles, any R
// -- and the batch keeps its own limits (one request tile at least, 32768 at most, 1 GiB of
// planes unless that is less than a tile).  Built with -fsanitize=address,undefined and run by
// tests/test_planes_sizing.py.
#include <cstdio>
#include <vector>

#include "../../boom_amd/csrc/planes_sizing.h"

using namespace boom_amd;
typedef unsigned __int128 u128;

static int failures = 0;

static void check(size_t chains, int64_t n, size_t p) {
  const size_t np = cols_planes(n);
  const int64_t batch = column_request_batch(chains, n, p);
  const size_t cap = column_planes_doubles(chains, n, p);
  auto bad = [&](const char *what) {
    std::printf("FAIL chains %zu n %lld p %zu: %s (planes %zu batch %lld capacity %zu)\n", chains, (long long)n, p,
                what, np, (long long)batch, cap);
    ++failures;
  };
  if (np != (size_t)((n + 2047) / 2048) || np < 1) bad("plane count");
  if (batch < 1 || batch > 32768) bad("batch out of [1, 32768]");
  if ((u128)batch > (u128)chains * p) bad("batch exceeds the number of vectors");
  if (batch < 64 && (u128)batch != (u128)chains * p) bad("batch below one request tile");
  if (batch > 64 && (u128)batch * np * p * 8 > ((u128)1 << 30)) bad("a batch's planes exceed 1 GiB");
  // the rows products: every chain in one launch
  if ((u128)cap < (u128)np * chains * p) bad("capacity below planes * chains * p");
  // the column launches of build_columns, for every request count a sweep can have
  const u128 all = (u128)chains * p;
  const u128 counts[] = {1, 63, 64, 65, (u128)batch - 1, (u128)batch, (u128)batch + 1, all / 2, all};
  for (u128 R : counts) {
    if (R < 1 || R > all) continue;
    const u128 launch = R < (u128)batch ? R : (u128)batch;
    if ((u128)cap < (u128)np * launch * p) bad("capacity below planes * min(batch, R) * p");
  }
  // (no wrap-around in the size_t arithmetic of the header)
  const u128 rows = (u128)batch > (u128)chains ? (u128)batch : (u128)chains;
  if ((u128)cap != rows * np * p) bad("capacity is not max(batch, chains) * planes * p");
}

int main() {
  // the shapes that the batch-sized workspace did not cover, then a grid around every edge
  check(1024, 100000, 4096);
  check(5243, 50000, 1024);
  check(33000, 64, 2);
  check(40000, 64, 4);
  const std::vector<size_t> chains = {1, 2, 6, 63, 64, 65, 1024, 5243, 32767, 32768, 32769, 33000, 40000, 65535, 1000000};
  const std::vector<int64_t> ns = {1, 17, 64, 2047, 2048, 2049, 4100, 50000, 100000, 10000000};
  const std::vector<size_t> ps = {1, 2, 4, 5, 127, 128, 129, 260, 1024, 4096, 65535};
  int shapes = 4;
  for (size_t c : chains)
    for (int64_t n : ns)
      for (size_t p : ps) {
        check(c, n, p);
        ++shapes;
      }
  std::printf("%d shapes, %d failures\n", shapes, failures);
  return failures ? 1 : 0;
}
