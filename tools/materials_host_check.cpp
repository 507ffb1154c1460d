// The host-side record patch of pt_materials_update (csrc/materials_host.h) as a stand-alone program: random records,
// objIndex values that name no object among them, against a restatement written the slow way; then ranges at the
// ends of the buffer and of the table. Build and run, with the sanitizers if wanted:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o /tmp/materials_host_check tools/materials_host_check.cpp && /tmp/materials_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../path-tracing-svgf_amd/csrc/materials_host.h"

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      printf("FAILED %s (line %d)\n", #c, __LINE__);            \
      ++failures;                                               \
    }                                                           \
  } while (0)

// tests/materials_ref.py, object by object
static std::vector<float> restated(std::vector<float> rec, const std::vector<float>& table, int first, int count) {
  const size_t n = rec.size() / 45;
  for (int k = 0; k < count; ++k)
    for (size_t i = 0; i < n; ++i)
      if (rec[i * 45 + 42] == (float)(first + k))
        for (int j = 0; j < 18; ++j) rec[i * 45 + 18 + j] = table[(size_t)k * 18 + j];
  return rec;
}

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

int main() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(-2.0f, 2.0f);
  const float odd[] = {0.5f, -1.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(), 1.0000001f,
                       std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 16777216.0f,
                       3.0e9f, -3.0e9f};
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)17, (size_t)1000}) {
    std::vector<float> rec(n * 45);
    for (float& f : rec) f = u(rng);
    for (size_t i = 0; i < n; ++i) rec[i * 45 + 42] = i % 3 == 0 ? odd[(i / 3) % 10] : (float)(rng() % 7);
    for (int first : {0, 1, 3, 6, 100}) {
      for (int count : {1, 2, 4, 4096}) {
        std::vector<float> table((size_t)count * 18);
        for (float& f : table) f = u(rng);
        std::vector<float> got = rec;
        ptapi::patch_records_host(got.data(), n, table.data(), first, count);
        CHECK(same_bits(got, restated(rec, table, first, count)));
        for (size_t i = 0; i < n; ++i) {  // nothing but floats 18 .. 35 ever changes
          CHECK(memcmp(&got[i * 45], &rec[i * 45], 18 * sizeof(float)) == 0);
          CHECK(memcmp(&got[i * 45 + 36], &rec[i * 45 + 36], 9 * sizeof(float)) == 0);
        }
      }
    }
  }
  {  // the last object of the largest range, in the last record; the first past it is left alone
    const int first = (1 << 24) - 4096, count = 4096;
    std::vector<float> rec(2 * 45, 1.0f), table((size_t)count * 18, 7.0f);
    rec[42] = (float)((1 << 24) - 1);
    rec[45 + 42] = 16777216.0f;
    std::vector<float> got = rec;
    ptapi::patch_records_host(got.data(), 2, table.data(), first, count);
    CHECK(got[18] == 7.0f && got[35] == 7.0f && got[17] == 1.0f && got[36] == 1.0f);
    CHECK(memcmp(&got[45], &rec[45], 45 * sizeof(float)) == 0);
  }
  printf(failures ? "materials_host_check: %d failures\n" : "materials_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
