// orcgpu_decomp_plan.inc -- the block decompressors' tables, as far as they are a function of ONE staged stream: built once, when
// the stream is staged (build_stream_tables, from scan_chunks), in the layout the kernels read (device/decomp_tables.h), with
// every pointer and index relative to the stream.  A decode call only counts (tables_count), hands out bases and copies the
// prebuilt entries into its pinned table while rebasing them (tables_fill): one linear pass of adds.
//
// The unit is the STREAM, not the stripe: a call decodes the streams of the columns it was asked for, and a call split over
// column lanes gives every lane a subset of every stripe's streams.  A stripe's tables are those of its streams; they live in
// the staged stripe (StagedStream::tables), hold no pointer at all, and go when it does.
//
// No HIP in this file and nothing of the context: tests/hostcheck/decomp_plan_check.cpp compiles it for the host, under
// AddressSanitizer, against a plain builder that fills a call's tables from the chunk lists directly.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "device/decomp_tables.h"

namespace {

struct ChunkInfo {
  uint64_t src_off;  // offset of the chunk payload inside the stream
  uint32_t len;
  uint32_t original;
  uint32_t plain_cap;  // bytes the chunk can expand to (exact for original and Snappy chunks, and for Zstandard frames that state their size)
  int32_t zparse = -1; // Zstandard: index into StagedStream::zchunks
};

// Blocks and chunks are taken by the kernels in the order of their sequence counts, the largest first (the longest serial chains
// start when the kernel does), position ascending within a count.  Counts are clamped to 2^18: what lies above shares the top
// bucket, in position order.
constexpr uint32_t kCountBuckets = 1u << 18;
inline uint32_t count_key(uint64_t c) { return (uint32_t)std::min<uint64_t>(c, kCountBuckets - 1); }

// Scratch of a chunk's own (0: none).  Snappy / LZ4: one 8-byte record per token (lz_parse.h) -- a Snappy element takes two
// bytes or more; an LZ4 sequence (two records) three, but for the last one.  DEFLATE: literal bytes + 12-byte match records
// (inflate_parse.h); a match yields three bytes or more
inline uint64_t chunk_record_bytes(int compression, const ChunkInfo& c) {
  if (c.original) return 0;
  if (compression == ORCGPU_COMP_SNAPPY) return 8ull * (c.len / 2 + 2);
  if (compression == ORCGPU_COMP_LZ4) return 8ull * (2 * (c.len / 3 + 1) + 2);
  if (compression == ORCGPU_COMP_ZLIB) return (((uint64_t)c.plain_cap + 16 + 15) & ~15ull) + 12ull * (c.plain_cap / 3 + 2) + 16;
  return 0;
}

// Sequence scratch of a block: ((nseq + 3) & ~3) sequences and 16 bytes.  One wavefront per block writes three arrays of that
// many 4-byte entries (12 bytes a sequence), one lane per block 8-byte records (padded to an even count: zstd_lanes.h)
constexpr uint32_t kSeqBytesArrays = 12, kSeqBytesPacked = 8;
inline uint32_t seq_round(uint32_t nseq) { return (nseq + 3u) & ~3u; }

// One stream's part of the tables.  Relative fields, and what a call adds to them:
//   ChunkDesc::src, ZBlock::src        offset in the stripe's arena              + the arena
//   ChunkDesc::dst                     offset in the stream's plain buffer       + that buffer
//   ChunkDesc::scratch, ZBlock::lit_out / seq_out   null, or 1 + the offset in the stream's scratch with 8-byte sequences
//                                      + the scratch base - 1 (+ 4 bytes per sequence reserved in front of it: seq_before, when the call writes arrays)
//   ChunkDesc::first_item              + the stream's first item;  ChunkDesc::stream = 0   + the stream's index
//   ZBlock::chunk                      + the stream's first chunk
//   ZItem::zblock, ZItem::seq_packed   0: the block's rank in the call and the call's mode
struct StreamTables {
  std::vector<ChunkDesc> chunks;
  std::vector<ZItem> items;             // every block of every Zstandard chunk, chunk after chunk
  std::vector<ZBlock> zblocks;          // the compressed blocks, most sequences first, position ascending within a count
  std::vector<uint32_t> zb_item;        // per entry of zblocks: its item
  std::vector<uint64_t> zb_seq_before;  // per entry of zblocks: rounded sequences (seq_round) whose scratch lies in front of the block's
  std::vector<std::pair<uint32_t, uint32_t>> zb_hist;     // zblocks' counts, descending: (count_key, blocks that have it)
  std::vector<uint32_t> chunk_order;    // the chunks, most sequences first, index ascending within a count
  std::vector<std::pair<uint32_t, uint32_t>> chunk_hist;  // (count_key of a chunk's sequences, chunks that have it), descending
  uint32_t n_chains = 0;                // blocks that have sequences
  uint32_t max_nseq = 0;                // the longest chain
  uint64_t total_seq = 0;
  uint64_t seq_rounded = 0;             // sum of seq_round over the blocks
  uint64_t scratch8 = 0;                // bytes of record, literal and sequence scratch with 8-byte sequences (a 16-aligned base is assumed)
  uint64_t plain_cap = 0;               // sum of the chunks' slots
  uint64_t scratch_bytes(uint32_t seq_bytes) const { return scratch8 + (uint64_t)(seq_bytes - kSeqBytesPacked) * seq_rounded; }
};

void build_stream_tables(const std::vector<ChunkInfo>& chunks, const std::vector<ZChunkParse>& zchunks, int compression, uint64_t arena_off, uint32_t codec_error,
                         StreamTables& T) {
  T = StreamTables{};
  T.chunks.reserve(chunks.size());
  {
    size_t n_items = 0;
    for (auto& zp : zchunks) n_items += zp.items.size();
    T.items.reserve(n_items);
  }
  auto rel = [](uint64_t v) { return reinterpret_cast<uint8_t*>((uintptr_t)v); };
  std::vector<ZBlock> zb_pos;           // the blocks in position order, with their keys, items and scratch
  std::vector<uint32_t> zb_pos_item;
  std::vector<uint64_t> zb_pos_before;
  std::vector<uint32_t> chunk_keys;
  uint64_t slot = 0, sc = 0;
  auto take = [&](uint64_t n) {
    sc = (sc + 15) & ~15ull;
    const uint64_t r = sc;
    sc += n;
    return r;
  };
  for (auto& c : chunks) {
    const uint32_t ci = (uint32_t)T.chunks.size();
    ChunkDesc cd;
    memset(&cd, 0, sizeof(cd));
    cd.src = rel(arena_off + c.src_off);
    cd.dst = rel(slot);
    const uint64_t rec = chunk_record_bytes(compression, c);
    if (rec) cd.scratch = rel(take(rec) + 1);
    cd.src_len = c.len;
    cd.dst_cap = c.plain_cap;
    cd.kind = c.original ? 0u : (uint32_t)compression;
    cd.first_item = (uint32_t)T.items.size();
    uint64_t chunk_seq = 0;
    if (c.zparse >= 0) {
      const ZChunkParse& zp = zchunks[c.zparse];
      cd.n_items = (uint32_t)zp.items.size();
      if (zp.bad) cd.status = codec_error;
      for (const ZItemH& ih : zp.items) {
        ZItem zi;
        memset(&zi, 0, sizeof(zi));
        zi.kind = ih.kind;
        zi.flags = ih.flags;
        zi.fcs = ih.fcs;
        zi.ck_off = ih.ck_off;
        if (ih.kind == 0) {
          zi.size = ih.size;
          zi.src_off = ih.off;
        } else if (ih.kind == 1) {
          zi.size = ih.size;
          zi.src_off = ih.rle_byte;
        } else {
          zi.lit_kind = ih.lit_type == 0 ? 0u : (ih.lit_type == 1 ? 1u : 2u);
          zi.lit_off = ih.lit_type == 1 ? (uint32_t)ih.rle_byte : ih.off + ih.lit_hdr;
          zi.litn = ih.lit_regen;
          zi.size = ih.block_max;
          zi.nseq = ih.nseq;
          ZBlock zb;
          memset(&zb, 0, sizeof(zb));
          zb.src = cd.src;
          zb_pos_before.push_back(T.seq_rounded);
          if (ih.lit_type >= 2) zb.lit_out = rel(take((uint64_t)ih.lit_regen + 16) + 1);
          if (ih.nseq) {
            zb.seq_out = reinterpret_cast<uint32_t*>(rel(take((uint64_t)kSeqBytesPacked * seq_round(ih.nseq) + 16) + 1));
            T.seq_rounded += seq_round(ih.nseq);
            T.n_chains++;
          }
          zb.chunk = ci;
          zb.content_off = ih.off;
          zb.content_end = ih.off + ih.size;
          zb.lit_type = ih.lit_type;
          zb.lit_streams = ih.lit_streams;
          zb.lit_hdr = ih.lit_hdr;
          zb.lit_regen = ih.lit_regen;
          zb.lit_comp = ih.lit_comp;
          zb.nseq = ih.nseq;
          zb.seq_off = ih.seq_off;
          if (ih.lit_type == 3) {
            const ZItemH& def = zp.items[ih.huf_def];
            zb.huf_off = def.off + def.lit_hdr;
            zb.huf_end = zb.huf_off + def.lit_comp;
          }
          for (int w = 0; w < 3; w++) {
            const ZItemH& def = ih.nseq && ih.tab_def[w] >= 0 ? zp.items[ih.tab_def[w]] : ih;
            zb.tab_off[w] = def.seq_off;
            zb.tab_end[w] = def.off + def.size;
          }
          zb_pos.push_back(zb);
          zb_pos_item.push_back((uint32_t)T.items.size());
          chunk_seq += ih.nseq;
          T.total_seq += ih.nseq;
          T.max_nseq = std::max(T.max_nseq, ih.nseq);
        }
        T.items.push_back(zi);
      }
    }
    chunk_keys.push_back(count_key(chunk_seq));
    T.chunks.push_back(cd);
    slot += c.plain_cap;
  }
  T.plain_cap = slot;
  T.scratch8 = sc;
  // the orders: count descending, position ascending within a count
  auto order_desc = [](uint32_t n, auto key, std::vector<uint32_t>& order, std::vector<std::pair<uint32_t, uint32_t>>& hist) {
    order.resize(n);
    for (uint32_t k = 0; k < n; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) > key(b); });
    hist.clear();
    for (uint32_t k = 0; k < n; k++) {
      if (hist.empty() || hist.back().first != key(order[k])) hist.push_back({key(order[k]), 0u});
      hist.back().second++;
    }
  };
  std::vector<uint32_t> zorder;
  order_desc((uint32_t)zb_pos.size(), [&](uint32_t k) { return count_key(zb_pos[k].nseq); }, zorder, T.zb_hist);
  T.zblocks.reserve(zorder.size());
  T.zb_item.reserve(zorder.size());
  T.zb_seq_before.reserve(zorder.size());
  for (uint32_t k : zorder) {
    T.zblocks.push_back(zb_pos[k]);
    T.zb_item.push_back(zb_pos_item[k]);
    T.zb_seq_before.push_back(zb_pos_before[k]);
  }
  order_desc((uint32_t)T.chunks.size(), [&](uint32_t k) { return chunk_keys[k]; }, T.chunk_order, T.chunk_hist);
}

// ---- a call -----------------------------------------------------------------------------------------------------------------
struct TableCounts {
  uint32_t n_streams = 0, n_chunks = 0, n_zblocks = 0, n_zitems = 0, n_zchains = 0;
  uint64_t total_seq = 0;
  std::vector<uint32_t> chunk0, item0;  // per stream: its first chunk and item in the call's tables
  std::vector<uint32_t> zb_at;          // per count_key: rank of the call's first block with that count (most sequences first)
  std::vector<uint32_t> chunk_at;       // per count_key of a chunk: place of the first such chunk in the execution order
};

// Adds up the streams of a call, in call order, and merges their orders: the histograms are added, a block's rank is then the
// first rank of its count plus the blocks with that count in the streams before it and in front of it in its own.
inline void ranks_of(const std::vector<std::pair<uint32_t, uint32_t>>* const* hists, size_t n, std::vector<uint32_t>& at) {
  uint32_t mx = 0;
  for (size_t k = 0; k < n; k++)
    if (!hists[k]->empty()) mx = std::max(mx, hists[k]->front().first);
  at.assign((size_t)mx + 1, 0);
  for (size_t k = 0; k < n; k++)
    for (auto& h : *hists[k]) at[h.first] += h.second;
  uint32_t r = 0;
  for (size_t key = at.size(); key-- > 0;) {
    const uint32_t c = at[key];
    at[key] = r;
    r += c;
  }
}
void tables_count(const StreamTables* const* t, size_t n, TableCounts& C) {
  C = TableCounts{};
  C.n_streams = (uint32_t)n;
  C.chunk0.resize(n);
  C.item0.resize(n);
  std::vector<const std::vector<std::pair<uint32_t, uint32_t>>*> zh(n), ch(n);
  for (size_t k = 0; k < n; k++) {
    C.chunk0[k] = C.n_chunks;
    C.item0[k] = C.n_zitems;
    C.n_chunks += (uint32_t)t[k]->chunks.size();
    C.n_zitems += (uint32_t)t[k]->items.size();
    C.n_zblocks += (uint32_t)t[k]->zblocks.size();
    C.n_zchains += t[k]->n_chains;
    C.total_seq += t[k]->total_seq;
    zh[k] = &t[k]->zb_hist;
    ch[k] = &t[k]->chunk_hist;
  }
  ranks_of(zh.data(), n, C.zb_at);
  ranks_of(ch.data(), n, C.chunk_at);
}

struct StreamUse {   // what a call adds to a stream's tables
  const StreamTables* t;
  const uint8_t* arena;   // the staged arena of its stripe
  uint8_t* plain;         // the stream's plain buffer
  uint8_t* scratch;       // its record / literal / sequence scratch (scratch_bytes(seq_bytes) of it, 16-aligned), null when it needs none
  uint32_t len_idx, err_idx, framing_error, skip;
};

// The call's tables: hc[n_chunks], hstr[n_streams], hzb[n_zblocks], hzi[n_zitems], ord[n_chunks] (the execution order).
void tables_fill(const StreamUse* use, const TableCounts& C, bool packed, ChunkDesc* hc, StreamDesc* hstr, ZBlock* hzb, ZItem* hzi, uint32_t* ord) {
  std::vector<uint32_t> zb_at = C.zb_at, chunk_at = C.chunk_at;
  const uint64_t extra = packed ? 0u : kSeqBytesArrays - kSeqBytesPacked;
  auto at = [](const void* base, const void* rel, uint64_t more = 0) { return (uintptr_t)base + (uintptr_t)rel + (uintptr_t)more; };
  for (uint32_t si = 0; si < C.n_streams; si++) {
    const StreamUse& u = use[si];
    const StreamTables& T = *u.t;
    const uint32_t c0 = C.chunk0[si], i0 = C.item0[si];
    StreamDesc& sd = hstr[si];
    sd.first_chunk = c0;
    sd.n_chunks = (uint32_t)T.chunks.size();
    sd.len_idx = u.len_idx;
    sd.err_idx = u.err_idx;
    sd.base = u.plain;
    sd.framing_error = u.framing_error;
    sd.skip = u.skip;
    const size_t nc = T.chunks.size();
    if (nc) memcpy(hc + c0, T.chunks.data(), nc * sizeof(ChunkDesc));
    for (size_t k = 0; k < nc; k++) {
      ChunkDesc& cd = hc[c0 + k];
      cd.src = reinterpret_cast<const uint8_t*>(at(u.arena, cd.src));
      cd.dst = reinterpret_cast<uint8_t*>(at(u.plain, cd.dst));
      if (cd.scratch) cd.scratch = reinterpret_cast<uint8_t*>(at(u.scratch, cd.scratch) - 1);
      cd.stream = si;
      cd.first_item += i0;
    }
    if (!T.items.empty()) memcpy(hzi + i0, T.items.data(), T.items.size() * sizeof(ZItem));
    size_t j = 0;
    for (auto& h : T.zb_hist) {
      const uint32_t r0 = zb_at[h.first];
      zb_at[h.first] += h.second;
      memcpy(hzb + r0, T.zblocks.data() + j, (size_t)h.second * sizeof(ZBlock));
      for (uint32_t q = 0; q < h.second; q++, j++) {
        ZBlock& zb = hzb[r0 + q];
        const uint64_t more = extra * T.zb_seq_before[j];
        zb.src = reinterpret_cast<const uint8_t*>(at(u.arena, zb.src));
        if (zb.lit_out) zb.lit_out = reinterpret_cast<uint8_t*>(at(u.scratch, zb.lit_out, more) - 1);
        if (zb.seq_out) zb.seq_out = reinterpret_cast<uint32_t*>(at(u.scratch, zb.seq_out, more) - 1);
        zb.chunk += c0;
        ZItem& zi = hzi[i0 + T.zb_item[j]];
        zi.zblock = r0 + q;
        zi.seq_packed = packed ? 1u : 0u;
      }
    }
    j = 0;
    for (auto& h : T.chunk_hist) {
      const uint32_t r0 = chunk_at[h.first];
      chunk_at[h.first] += h.second;
      for (uint32_t q = 0; q < h.second; q++, j++) ord[r0 + q] = c0 + T.chunk_order[j];
    }
  }
}

}  // namespace
