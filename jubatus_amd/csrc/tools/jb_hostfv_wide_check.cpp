// Stand-alone run of the native wide converter (csrc/native/jb_hostfv_wide.hpp)
// over packed rule tables, for instrumented builds: HostFvWide is a header the
// Python runtime loads, and a sanitizer sees it only in a program of its own.
//   jb_hostfv_wide_check <tables> <body> [update]
// <tables>: what fv_converter/gpu_path.py WideRuleTable packs, little-endian:
//   uint64 H | int32 n_srules, n_nrules, n_crules, blob_len |
//   32 x n_srules | 32 x n_nrules | 64 x n_crules | blob
// <body>: one msgpack list<datum>. Prints one line "idx bits name" per feature
// (bits: the float32 value in hex; the name from the names sink) and "--"
// after every datum; `update` counts the datums into the document statistics.
// Exit status 0 ok, 1 malformed input, 2 usage.
#include <stdio.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "jb_hostfv_wide.hpp"

static bool slurp(const char* path, std::vector<uint8_t>* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: jb_hostfv_wide_check <tables> <body> [update]\n");
    return 2;
  }
  std::vector<uint8_t> t, body;
  if (!slurp(argv[1], &t) || !slurp(argv[2], &body) || t.size() < 24) return 2;
  const bool update = argc > 3 && std::string(argv[3]) == "update";
  uint64_t H;
  int32_t n[4];
  memcpy(&H, t.data(), 8);
  memcpy(n, t.data() + 8, 16);
  if (n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0 || H == 0) return 2;
  const size_t so = 24, no = so + 32 * (size_t)n[0], co = no + 32 * (size_t)n[1];
  const size_t bo = co + 64 * (size_t)n[2];
  if (t.size() != bo + (size_t)n[3]) return 2;
  // copies of their exact sizes: a read past a table is a read past an allocation
  const std::vector<uint8_t> sr(t.begin() + so, t.begin() + no), nr(t.begin() + no, t.begin() + co),
      cr(t.begin() + co, t.begin() + bo), blob(t.begin() + bo, t.end());
  jb::HostFvWide h(sr.data(), n[0], nr.data(), n[1], cr.data(), n[2], blob.data(), blob.size(), H);
  std::vector<int64_t> df, diff;
  int64_t counts[4] = {0, 0, 0, 0};
  if (h.needs_weights()) {
    df.assign(H, 0);
    diff.assign(H, 0);
    h.set_weights(df.data(), diff.data(), counts);
  }
  std::string names;
  std::vector<int64_t> name_end, spans;
  h.set_sinks(&names, &name_end, &spans);
  jb::Cursor c{body.data(), body.data() + body.size()};
  uint32_t cnt;
  if (!c.array(&cnt)) return 1;
  std::vector<int32_t> idx(1 << 16);
  std::vector<float> val(idx.size());
  h.begin();
  for (uint32_t i = 0; i < cnt; ++i) {
    int64_t slots = 0;
    // (2: a datum above 65536 features, not what this tool is for)
    if (h.hash_datum(c, idx.data(), val.data(), (int64_t)idx.size(), &slots, update)) return 1;
    const size_t first = name_end.size() - (size_t)slots;
    for (size_t s = 0; s < (size_t)slots; ++s) {
      uint32_t bits;
      memcpy(&bits, &val[s], 4);
      const int64_t b0 = first + s ? name_end[first + s - 1] : 0;
      printf("%d %08x %.*s\n", idx[s], bits, (int)(name_end[first + s] - b0), names.data() + b0);
    }
    printf("--\n");
  }
  if (h.needs_weights())
    printf("counts %lld %lld\n", (long long)counts[0], (long long)counts[1]);
  return 0;
}
