// writer_host_check.cpp -- the ArrowWriter's device-free host code (orc_rust_amd/csrc/orcgpu_writer_host.inc, the very text
// liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Reads one case per line on
// stdin and prints one result line each; tests/test_writer_host_sanitized.py judges them against the project's models.
//   lower HEX | upper HEX            wr_lower_bound / wr_upper_bound of the bytes ("none": no upper bound)
//   dec HI LO SCALE                  wr_decimal_string of the 128-bit two's complement value
//   int FMT N {count min max sum_hi sum_lo has_null}*N  the groups' records of a column of Arrow format FMT merged ->
//   dbl FMT N {count min max sum sum_lo big big_lo has_nan has_null}*N      ColumnStatistics, hex (doubles as hex bit patterns)
//   meta HEX                         wr_metadata of the blob -> hex
//   tree | refuse NAME               the column tree of the built-in schema; the code a built-in field is refused with
//   streams KIND ELEM PRESENT DICT INDEXED   wr_streams of such a column
#include <cinttypes>
#include <iostream>
#include <sstream>

#include "../../orc_rust_amd/csrc/orcgpu_writer_host.inc"

static std::string unhex(const std::string& h) {
  std::string out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out += (char)strtoul(h.substr(i, 2).c_str(), nullptr, 16);
  return out;
}
static std::string hex(const void* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string out;
  for (size_t i = 0; i < n; i++) out += d[((const uint8_t*)p)[i] >> 4], out += d[((const uint8_t*)p)[i] & 15];
  return out.empty() ? "-" : out;
}
static double bits_double(const std::string& h) {
  const uint64_t u = strtoull(h.c_str(), nullptr, 16);
  double v;
  memcpy(&v, &u, 8);
  return v;
}
static WrField field(const char* fmt, const char* name, std::vector<WrField> kids = {}) {
  WrField f;
  f.format = fmt;
  f.name = name;
  f.kids = std::move(kids);
  return f;
}
// every supported type once, a Map of a Struct of a List among them
static std::vector<WrField> all_types() {
  WrField entries = field("+s", "entries", {field("u", "key"), field("+s", "value", {field("+l", "l", {field("i", "item")}), field("g", "x")})});
  return {field("b", "bool"), field("c", "i8"), field("s", "i16"), field("i", "i32"), field("l", "i64"), field("f", "f32"), field("g", "f64"),
          field("u", "s"), field("U", "ls"), field("z", "bin"), field("Z", "lbin"), field("tsn:", "ts"), field("tsu:UTC", "tz"), field("d:15,2", "dec"),
          field("+m", "m", {entries}), field("+L", "ll", {field("l", "item")})};
}
static WrField refused(const std::string& name) {
  if (name == "fixed_size_list") return field("+w:3", "f", {field("i", "item")});
  if (name == "dictionary") {
    WrField f = field("i", "f");
    f.dictionary = true;
    return f;
  }
  if (name == "decimal_below_list") return field("+l", "f", {field("d:10,2", "item")});
  if (name == "map_without_entries") return field("+m", "f", {field("u", "key")});
  return field(name.c_str(), "f");  // a format: d:39,2  d:5,6  d:10,2,256
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a;
    in >> cmd;
    if (cmd == "lower" || cmd == "upper") {
      in >> a;
      const std::string s = unhex(a);
      std::string out;
      if (cmd == "lower") out = wr_lower_bound(s);
      else if (!wr_upper_bound(s, out)) {
        printf("none\n");
        continue;
      }
      printf("%s\n", hex(out.data(), out.size()).c_str());
    } else if (cmd == "dec") {
      uint64_t hi, lo;
      uint32_t scale;
      in >> hi >> lo >> scale;
      printf("%s\n", wr_decimal_string((__int128)(((unsigned __int128)hi << 64) | lo), scale).c_str());
    } else if (cmd == "int" || cmd == "dbl") {
      int n;
      in >> a >> n;
      WrCol c;
      if (!wr_column_of(a.c_str(), c)) return 2;
      WrStat all;
      for (int g = 0; g < n; g++) {
        IxRec r{};
        std::string mn, mx, s0, s1, b0, b1;
        in >> r.count >> mn >> mx >> s0 >> s1;
        if (cmd == "dbl") in >> b0 >> b1 >> r.has_nan;
        in >> r.has_null;
        if (cmd == "int") {
          r.imin = strtoll(mn.c_str(), nullptr, 10), r.imax = strtoll(mx.c_str(), nullptr, 10);
          r.sum_hi = strtoll(s0.c_str(), nullptr, 10), r.sum_lo = strtoull(s1.c_str(), nullptr, 10);
        } else {
          r.dmin = bits_double(mn), r.dmax = bits_double(mx), r.dsum = bits_double(s0), r.dsum_lo = bits_double(s1);
          r.dbig = bits_double(b0), r.dbig_lo = bits_double(b1);
        }
        wr_stat_merge(all, wr_stat_of(c, r, nullptr));
      }
      const PbOut m = wr_stat_msg(&c, all);
      printf("%s\n", hex(m.b.data(), m.b.size()).c_str());
    } else if (cmd == "meta") {
      in >> a;
      const std::string blob = unhex(a), got = wr_metadata(blob.data());
      printf("%s\n", hex(got.data(), got.size()).c_str());
    } else if (cmd == "tree") {
      WrTree t;
      std::string err;
      const int rc = wr_tree_of(err, all_types(), t);
      printf("%d %zu %d", rc, t.cols.size(), (int)t.nested);
      for (auto& c : t.cols) printf(" %d,%d,%d,%d", c.orc_kind, c.encoding, c.parent, c.child);
      printf("\n");
    } else if (cmd == "refuse") {
      in >> a;
      WrTree t;
      std::string err;
      printf("%d\n", wr_tree_of(err, {refused(a)}, t));
    } else if (cmd == "streams") {
      WrCol c;
      int present, dict, indexed;
      in >> c.stream_kind >> c.elem >> present >> dict >> indexed;
      c.present = present, c.dict = dict;
      c.rows = 100, c.n_valid = 90, c.n_bytes = 700, c.dict_size = 4, c.dict_bytes = 20;
      WrStream s[WR_MAX_STREAMS];
      const int n = wr_streams(c, wr_counts(c), indexed != 0, s);
      printf("%d", n - present);
      for (int i = 0; i < n; i++) printf(" %d,%d,%d,%d,%d,%" PRIu64, s[i].stream, s[i].enc, s[i].is_signed, s[i].width, s[i].pos_mode, s[i].n);
      printf("\n");
    } else {
      printf("?\n");
    }
  }
  // the byte builders, run for the sanitizers' sake: an indexed two-column stripe and the tail of its file
  WrTree t;
  std::string err;
  wr_tree_of(err, {field("l", "a"), field("u", "s")}, t);
  std::vector<IxRec> recs(2);
  recs[0].count = recs[1].count = 3;
  recs[1].smin_len = recs[1].smax_len = 1;
  const uint64_t pos[16] = {0};
  std::vector<WrStat> stripe;
  const auto index = wr_row_index(t.cols, 3, 1000, 1, recs.data(), pos, (const uint8_t*)"ab", {{{0, 2}}, {{1, 1}, {2, 2}}}, true, 64, stripe);
  const auto footer = wr_stripe_footer(t.cols, index, {{ORCGPU_S_DATA, 1, 0}, {ORCGPU_S_DATA, 2, 0}, {ORCGPU_S_LENGTH, 2, 0}}, {5, 3, 4}, true, 64);
  const auto tail = wr_tail(t.cols, t.root_kids, {WrStripe{3, 12, footer.size(), 3, 0}}, {stripe}, 1000, ORCGPU_COMP_SNAPPY, 64);
  printf("built %zu %zu %zu\n", index.size(), footer.size(), tail.size());
  return 0;
}
