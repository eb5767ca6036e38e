// orcgpu_selection.inc -- RowSelection stepping, PURE C++ (no HIP): the stepping of NaiveStripeDecoder::next_with_row_selection
// (array_decoder/mod.rs:302-365), RowSelection's normalisation, split_off and intersection (row_selection.rs:278-314, :466-482).
// Included by orcgpu_select.inc (the product) and by tests/hostcheck/hostcheck.cpp (the sanitizer build of the host layer).
#pragma once
namespace {

struct RowSel {
  uint64_t row_count;
  bool skip;
};

// impl From<Vec<RowSelector>> for RowSelection (row_selection.rs:466-482): empty selectors dropped, neighbours of a kind merged
std::vector<RowSel> sel_normalise(const orcgpu_row_selector* in, uint32_t n) {
  std::vector<RowSel> out;
  for (uint32_t i = 0; i < n; i++) {
    if (!in[i].row_count) continue;
    const bool skip = in[i].skip != 0;
    if (!out.empty() && out.back().skip == skip) out.back().row_count += in[i].row_count;
    else out.push_back(RowSel{in[i].row_count, skip});
  }
  return out;
}
uint64_t sel_row_count(const std::vector<RowSel>& s) {
  uint64_t t = 0;
  for (auto& x : s) t += x.row_count;
  return t;
}
// RowSelection::split_off (row_selection.rs:278-314): the first row_count rows leave `s` and are returned
std::vector<RowSel> sel_split_off(std::vector<RowSel>& s, uint64_t row_count) {
  uint64_t total = 0;
  size_t idx = s.size();
  for (size_t i = 0; i < s.size(); i++) {
    total += s[i].row_count;
    if (total > row_count) {
      idx = i;
      break;
    }
  }
  if (idx == s.size()) {
    std::vector<RowSel> all;
    all.swap(s);
    return all;
  }
  std::vector<RowSel> remaining(s.begin() + idx, s.end());
  s.resize(idx);
  const uint64_t overflow = total - row_count;
  if (remaining[0].row_count != overflow) s.push_back(RowSel{remaining[0].row_count - overflow, remaining[0].skip});
  remaining[0].row_count = overflow;
  s.swap(remaining);
  return remaining;
}
// Rows of a stripe that both selections select (rows behind the end of a selection are not selected by it)
std::vector<RowSel> sel_intersect(const std::vector<RowSel>& a, const std::vector<RowSel>& b, uint64_t n_rows) {
  std::vector<RowSel> out;
  size_t ia = 0, ib = 0;
  uint64_t ra = 0, rb = 0, at = 0;  // rows of a[ia] / b[ib] already consumed
  while (at < n_rows) {
    while (ia < a.size() && ra == a[ia].row_count) ia++, ra = 0;
    while (ib < b.size() && rb == b[ib].row_count) ib++, rb = 0;
    const uint64_t la = ia < a.size() ? a[ia].row_count - ra : n_rows - at, lb = ib < b.size() ? b[ib].row_count - rb : n_rows - at;
    const bool sa = ia < a.size() ? !a[ia].skip : false, sb = ib < b.size() ? !b[ib].skip : false;
    const uint64_t step = std::min(std::min(la, lb), n_rows - at);
    if (!step) break;
    const bool skip = !(sa && sb);
    if (!out.empty() && out.back().skip == skip) out.back().row_count += step;
    else out.push_back(RowSel{step, skip});
    if (ia < a.size()) ra += step;
    if (ib < b.size()) rb += step;
    at += step;
  }
  return out;
}
// next_with_row_selection, run to the end of the stripe: the batches it yields as row ranges.  (Literal restatement, including
// that a select run longer than batch_size is not shortened by what it has yielded: mod.rs:337-347 compares the rows of ONE
// step with the selector's row_count.)
std::vector<SelBatch> sel_batches(const std::vector<RowSel>& sel, uint64_t number_of_rows, uint64_t batch_size) {
  std::vector<SelBatch> out;
  uint64_t index = 0;
  size_t si = 0;
  while (si < sel.size()) {
    const uint64_t row_count = sel[si].row_count;
    const uint64_t remaining = number_of_rows - index;
    if (sel[si].skip) {
      const uint64_t actual = std::min(row_count, remaining);
      if (!actual) {
        si++;
        continue;
      }
      index += actual;
      if (actual >= row_count) si++;
    } else {
      const uint64_t actual = std::min(std::min(row_count, batch_size), remaining);
      if (!actual) {
        si++;
        continue;
      }
      out.push_back(SelBatch{index, (uint32_t)actual, 0});
      index += actual;
      if (actual >= row_count) si++;
    }
  }
  return out;
}

}  // namespace
