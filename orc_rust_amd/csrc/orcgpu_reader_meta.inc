// orcgpu_reader_meta.inc -- the file reader's metadata through the GPU: compressed file tails, stripe footers and ROW_INDEX /
// BLOOM_FILTER streams are expanded with the SAME GPU block decompressors as the data streams (there is no CPU codec in the
// product), then parsed by orcgpu_meta.inc.
//
//   read_metadata                    src/reader/metadata.rs:180-247 (PostScript, Footer)
//   Decompressor::read_to_end        src/reader/metadata.rs:323-337
//   Stripe::read_row_indexes         src/stripe.rs:266-309, row_index.rs:204-330
#include <cstdio>
#include <memory>

#include "orcgpu_meta.inc"
namespace orcgpu_host {

struct SectionCopy {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t n;
};
__global__ void sections_pack_kernel(const SectionCopy* jobs) {
  const SectionCopy j = jobs[blockIdx.x];
  for (uint64_t i = threadIdx.x; i < j.n; i += blockDim.x) j.dst[i] = j.src[i];
}

// The expanded sections -> the host.  (They lie in the workspace a block size or more apart, whatever they hold: packed by a
// kernel, one copy back.)  o_dst[k]: where section k lies in the workspace S, h_scal[2 * k]: its length
int sections_copy_back(orcgpu_ctx* ctx, uint8_t* S, const std::vector<uint64_t>& o_dst, const std::vector<uint64_t>& h_scal, uint64_t o_pack, uint64_t pack_cap,
                       uint64_t o_jobs, std::vector<std::vector<uint8_t>>& outs) {
  const size_t n = o_dst.size();
  std::vector<SectionCopy> jobs(n);
  uint64_t total = 0;
  for (size_t k = 0; k < n; k++) {
    jobs[k] = SectionCopy{S + o_dst[k], S + o_pack + total, h_scal[2 * k]};
    total += h_scal[2 * k];
  }
  if (total > pack_cap) return ORCGPU_UNEXPECTED;
  std::vector<uint8_t> back(total);
  if (total) {
    HIP_TRY(ctx, ctx->upload(S + o_jobs, jobs.data(), n * sizeof(SectionCopy), ctx->stream));
    hipLaunchKernelGGL(sections_pack_kernel, dim3((uint32_t)n), dim3(256), 0, ctx->stream, reinterpret_cast<const SectionCopy*>(S + o_jobs));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(back.data(), S + o_pack, total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (size_t k = 0; k < n; k++) outs[k].assign(back.data() + (jobs[k].dst - (S + o_pack)), back.data() + (jobs[k].dst - (S + o_pack)) + jobs[k].n);
  return ORCGPU_OK;
}

// Expand ORC-framed metadata sections on the GPU (Decompressor::read_to_end, metadata.rs:323-337): the same path the stripe
// streams take -- host framing scan, block decoders, finalize (one contiguous plain stream each) --, all sections in one go.
int decompress_sections(orcgpu_ctx* ctx, const std::vector<std::vector<uint8_t>>& raws, int compression, uint64_t block_size,
                        std::vector<std::vector<uint8_t>>& outs) {
  const size_t n = raws.size();
  outs.assign(n, {});
  if (compression == ORCGPU_COMP_NONE) {
    for (size_t k = 0; k < n; k++) outs[k] = raws[k];
    return ORCGPU_OK;
  }
  if (!block_size) block_size = 262144;
  std::vector<StagedStream> ss(n);
  Plan P;
  std::vector<uint64_t> o_dst(n, 0);
  uint64_t src_total = 0;
  bool any = false;
  for (size_t k = 0; k < n; k++) {
    ss[k].column_id = (uint32_t)k;
    ss[k].kind = 0;
    ss[k].off = src_total;
    ss[k].len = raws[k].size();
    src_total += align_up(raws[k].size() + ORC_PAD);
    scan_chunks(raws[k].data(), raws[k].size(), compression, block_size, ss[k]);
    if (ss[k].framing_error) return ORCGPU_IO_ERROR;
    any = any || !ss[k].chunks.empty();
  }
  if (!any) return ORCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  orcgpu_staged tmp;
  tmp.ctx = ctx;
  tmp.desc.compression = compression;
  tmp.desc.block_size = block_size;
  const uint64_t o_src = P.scratch.take(src_total + ORC_PAD), o_scal = P.scratch.take(16 * n + 64);
  for (size_t k = 0; k < n; k++) {
    uint64_t cap_total = 0;
    for (auto& c : ss[k].chunks) cap_total += c.plain_cap;
    o_dst[k] = P.scratch.take(cap_total + ORC_PAD);
    if (!ss[k].chunks.empty()) P.decomp.push_back(DecompStream{&tmp, &ss[k], o_dst[k], (uint32_t)(2 * k), (uint32_t)(2 * k + 1)});
  }
  const uint64_t pack_cap = P.scratch.off - o_dst[0];
  const uint64_t o_pack = P.scratch.take(pack_cap + 64), o_jobs = P.scratch.take(n * sizeof(SectionCopy) + 64);
  DecompPlan DP;
  int rc = plan_decompress(P, DP);
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  ctx->upload_reset();
  if (!ctx->scratch.ensure(P.scratch.off + kAlign) || !ctx->ensure_pinned(DP.table_bytes + 64)) {
    set_err(ctx, "out of memory while expanding a metadata section");
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* S = ctx->scratch.p;
  tmp.dev = S + o_src;
  uint64_t* d_scal = reinterpret_cast<uint64_t*>(S + o_scal);
  HIP_TRY(ctx, hipMemsetAsync(d_scal, 0, 16 * n + 64, ctx->stream));
  {
    // (one copy up for all sections, one copy back for all of them: a copy of its own for each would cost more than the kernels)
    std::vector<uint8_t> up(src_total, 0);
    for (size_t k = 0; k < n; k++)
      if (!raws[k].empty()) memcpy(up.data() + ss[k].off, raws[k].data(), raws[k].size());
    HIP_TRY(ctx, ctx->upload(S + o_src, up.data(), up.size(), ctx->stream));
  }
  rc = launch_decompress(ctx, P, DP, S, d_scal, ctx->pinned);
  tmp.dev = nullptr;  // (borrowed: part of the workspace)
  if (rc) return rc;
  std::vector<uint64_t> h_scal(2 * n + 2, 0);
  HIP_TRY(ctx, hipMemcpyAsync(h_scal.data(), d_scal, 16 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < n; k++)
    if (h_scal[2 * k + 1]) {
      set_err(ctx, "a metadata chunk failed to decompress");
      return ORCGPU_BUILD_DECODER;
    }
  return sections_copy_back(ctx, S, o_dst, h_scal, o_pack, pack_cap, o_jobs, outs);
}
int decompress_section(orcgpu_ctx* ctx, const std::vector<uint8_t>& raw, int compression, uint64_t block_size, std::vector<uint8_t>& out) {
  std::vector<std::vector<uint8_t>> raws(1, raw), outs;
  int rc = decompress_sections(ctx, raws, compression, block_size, outs);
  if (!rc) out = std::move(outs[0]);
  return rc;
}

int read_metadata(orcgpu_ctx* ctx, ChunkReader& r, FileMetadata& md) {
  const uint64_t file_len = r.len();
  if (file_len == 0) {
    set_err(ctx, "empty file");
    return ORCGPU_OUT_OF_SPEC;
  }
  const uint64_t tail_len = std::min<uint64_t>(file_len, 16 * 1024);  // DEFAULT_FOOTER_SIZE (metadata.rs:60)
  std::vector<uint8_t> tail;
  if (!r.get_bytes(file_len - tail_len, tail_len, tail)) return ORCGPU_IO_ERROR;
  MetaErr e;
  uint64_t ps_len = 0, footer_length = 0;
  int rc = parse_postscript(tail.data(), tail.size(), md, ps_len, footer_length, e);
  if (rc) {
    if (e.msg[0]) set_err(ctx, "%s", e.msg);
    return rc;
  }
  const uint64_t footer_end = file_len - 1 - ps_len;
  if (footer_length > footer_end) return ORCGPU_OUT_OF_SPEC;
  std::vector<uint8_t> raw_footer;
  if (!r.get_bytes(footer_end - footer_length, footer_length, raw_footer)) return ORCGPU_IO_ERROR;
  std::vector<uint8_t> footer;
  rc = decompress_section(ctx, raw_footer, md.compression, md.block_size, footer);
  if (rc) return rc;
  rc = parse_footer(footer.data(), footer.size(), md, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int stripe_footer_raw(orcgpu_ctx* ctx, ChunkReader& r, const StripeInfo& si, std::vector<uint8_t>& raw) {
  MetaErr e;
  const int rc = stripe_footer_raw(r, si, raw, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int parse_stripe_footer(orcgpu_ctx* ctx, const StripeInfo& si, const std::vector<uint8_t>& plain, StripeFooter& sf) {
  MetaErr e;
  const int rc = parse_stripe_footer(si, plain, sf, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int read_stripe_footer(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const StripeInfo& si, StripeFooter& sf) {
  std::vector<uint8_t> raw, plain;
  int rc = stripe_footer_raw(ctx, r, si, raw);
  if (!rc) rc = decompress_section(ctx, raw, md.compression, md.block_size, plain);
  return rc ? rc : parse_stripe_footer(ctx, si, plain, sf);
}

// The footers of several stripes, their sections expanded by ONE call of the GPU decompressors (a call costs a launch chain and
// two host round trips however little it expands).  out[k] <- stripe infos[k]; the count of footers read is returned, and when
// that is short of infos.size(), *rc_out says why footer number `count` could not be read (ctx->err holds the message).
size_t read_stripe_footers(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const std::vector<const StripeInfo*>& infos,
                           std::vector<StripeFooter>& out, int* rc_out) {
  const size_t n = infos.size();
  out.assign(n, StripeFooter{});
  *rc_out = 0;
  std::vector<std::vector<uint8_t>> raws(n), plains;
  bool batched = n > 1;
  for (size_t k = 0; k < n && batched; k++) batched = stripe_footer_raw(ctx, r, *infos[k], raws[k]) == ORCGPU_OK;
  if (batched) batched = decompress_sections(ctx, raws, md.compression, md.block_size, plains) == ORCGPU_OK;
  for (size_t k = 0; k < n; k++) {
    // (anything wrong in the batch: one at a time, so that the stripes in front of the bad one are still read)
    int rc = batched ? parse_stripe_footer(ctx, *infos[k], plains[k], out[k]) : read_stripe_footer(ctx, r, md, *infos[k], out[k]);
    if (rc) {
      *rc_out = rc;
      return k;
    }
  }
  return n;
}

// Stripe::read_row_indexes (stripe.rs:266-309, row_index.rs:204-226): the ROW_INDEX streams of `columns`, expanded by the GPU
// decompressors in one go, parsed into position lists.  Columns without such a stream get no entry.
// want_stats: also the row groups' statistics and the columns' BLOOM_FILTER (else BLOOM_FILTER_UTF8) streams (row_index.rs:228-330)
int read_stripe_index(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, StripeFooter& sf, const std::vector<uint32_t>& columns, bool want_stats) {
  sf.index.clear();
  sf.index_read = true;
  std::vector<std::vector<uint8_t>> raws, plains;
  IndexSections is;
  int rc = index_gather(r, sf, columns, want_stats, raws, is);
  if (rc || raws.empty()) return rc;
  rc = decompress_sections(ctx, raws, md.compression, md.block_size, plains);
  return rc ? rc : index_parse(sf, is, plains, want_stats);
}

// The indexes of several stripes by ONE call of the GPU decompressors.  A stripe whose index cannot be read or parsed is left
// with none (index_read set): it is decoded whole.
void read_stripe_indexes(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const std::vector<StripeFooter*>& sfs,
                         const std::vector<uint32_t>& columns, bool want_stats) {
  std::vector<std::vector<uint8_t>> raws, plains;
  std::vector<IndexSections> is(sfs.size());
  bool batched = sfs.size() > 1;
  for (size_t k = 0; k < sfs.size() && batched; k++) batched = index_gather(r, *sfs[k], columns, want_stats, raws, is[k]) == ORCGPU_OK;
  if (batched && !raws.empty()) batched = decompress_sections(ctx, raws, md.compression, md.block_size, plains) == ORCGPU_OK;
  for (size_t k = 0; k < sfs.size(); k++) {
    StripeFooter& sf = *sfs[k];
    int rc;
    if (batched) {
      sf.index.clear();
      sf.index_read = true;
      rc = is[k].n ? index_parse(sf, is[k], plains, want_stats) : ORCGPU_OK;
    } else {
      rc = read_stripe_index(ctx, r, md, sf, columns, want_stats);  // (anything wrong in the batch: one stripe at a time)
    }
    if (rc) {
      sf.index.clear();
      sf.index_read = true;
    }
  }
}

}  // namespace orcgpu_host
