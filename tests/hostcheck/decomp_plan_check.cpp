// decomp_plan_check.cpp -- the decompressors' table builder (orc_rust_amd/csrc/orcgpu_decomp_plan.inc, the very text liborcgpu.so
// is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Streams are described by hand (chunk lists
// and parsed Zstandard blocks); their tables are built once (build_stream_tables, as at stage time), then merged and rebased for
// a number of calls (tables_count / tables_fill) and compared, field by field, with the tables of `reference_tables`: the
// builder a decode call used before the streams carried their tables -- one walk over the call's chunk lists, workspace taken
// block after block, a counting sort over the call's blocks.  Both Zstandard modes (sequence scratch of 12 and of 8 bytes).
// Prints one line per case; exit code 0 when every case agreed; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_zstd_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_decomp_plan.inc"

static const uint32_t kCodecError = 9;  // ORC_E_CODEC (device/rle_parse.h)

struct Stream {
  int compression = ORCGPU_COMP_ZSTD;
  uint64_t arena_off = 0;
  uint32_t skip = 0, framing_error = 0;
  std::vector<ChunkInfo> chunks;
  std::vector<ZChunkParse> zchunks;
  StreamTables tables;
};
struct Use {          // a stream in a call
  const Stream* st;
  const uint8_t* arena;
  uint8_t* plain;
  uint32_t len_idx, err_idx;
};
struct Tables {
  std::vector<ChunkDesc> chunks;
  std::vector<StreamDesc> streams;
  std::vector<ZBlock> zblocks;
  std::vector<ZItem> zitems;
  std::vector<uint32_t> order;
  uint32_t n_zchains = 0;
  uint64_t total_seq = 0, scratch_end = 0;
};

struct Bump16 {
  uint64_t off;
  uint64_t take(uint64_t n) {
    off = (off + 15) & ~15ull;
    const uint64_t r = off;
    off += n;
    return r;
  }
};

// ---- the reference: a call's tables from its chunk lists, the way plan_decompress / launch_decompress built them per call -----
template <class F>
static std::vector<uint32_t> order_by_count_desc(uint32_t n, F count) {
  constexpr uint32_t kBuckets = 1u << 18;
  std::vector<uint32_t> key(n), at;
  uint32_t mx = 0, live = 0;
  for (uint32_t k = 0; k < n; k++) {
    const int64_t c = count(k);
    key[k] = c < 0 ? 0xffffffffu : (uint32_t)std::min<int64_t>(c, kBuckets - 1);
    if (c >= 0) mx = std::max(mx, key[k]), live++;
  }
  at.assign((size_t)mx + 2, 0);
  for (uint32_t k = 0; k < n; k++)
    if (key[k] != 0xffffffffu) at[mx - key[k] + 1]++;
  for (uint32_t b = 0; b <= mx; b++) at[b + 1] += at[b];
  std::vector<uint32_t> out(live);
  for (uint32_t k = 0; k < n; k++)
    if (key[k] != 0xffffffffu) out[at[mx - key[k]]++] = k;
  return out;
}

static Tables reference_tables(const std::vector<Use>& call, uint8_t* S, uint64_t scratch0, uint32_t seq_bytes) {
  struct BlockPlan {
    uint32_t chunk;
    const ZItemH* item;
    uint64_t lit_off = ~0ull, seq_off = ~0ull;
    uint32_t zblock = 0;
  };
  Tables T;
  Bump16 scratch{scratch0};
  std::vector<BlockPlan> zitems;
  std::vector<uint32_t> chunk_first_item;
  std::vector<uint64_t> chunk_rec_off;
  uint32_t n_chunks = 0, n_zblocks = 0;
  for (auto& u : call) {
    const int k = u.st->compression;
    for (auto& c : u.st->chunks) {
      chunk_first_item.push_back((uint32_t)zitems.size());
      uint64_t rec = ~0ull;
      if (!c.original && k == ORCGPU_COMP_SNAPPY) rec = scratch.take(8ull * (c.len / 2 + 2));
      else if (!c.original && k == ORCGPU_COMP_LZ4) rec = scratch.take(8ull * (2 * (c.len / 3 + 1) + 2));
      else if (!c.original && k == ORCGPU_COMP_ZLIB) rec = scratch.take((((uint64_t)c.plain_cap + 16 + 15) & ~15ull) + 12ull * (c.plain_cap / 3 + 2) + 16);
      chunk_rec_off.push_back(rec);
      if (c.zparse >= 0)
        for (auto& it : u.st->zchunks[c.zparse].items) {
          BlockPlan bp;
          bp.chunk = n_chunks;
          bp.item = &it;
          if (it.kind == 2) {
            bp.zblock = n_zblocks++;
            if (it.lit_type >= 2) bp.lit_off = scratch.take((uint64_t)it.lit_regen + 16);
            if (it.nseq) bp.seq_off = scratch.take((uint64_t)seq_bytes * ((it.nseq + 3u) & ~3u) + 16);
          }
          zitems.push_back(bp);
        }
      n_chunks++;
    }
  }
  T.scratch_end = scratch.off;
  const uint32_t n_zitems = (uint32_t)zitems.size();
  std::vector<uint32_t> order = order_by_count_desc(n_zitems, [&](uint32_t k) -> int64_t { return zitems[k].item->kind == 2 ? (int64_t)zitems[k].item->nseq : -1; });
  for (uint32_t r = 0; r < order.size(); r++) {
    zitems[order[r]].zblock = r;
    T.total_seq += zitems[order[r]].item->nseq;
    if (zitems[order[r]].item->nseq) T.n_zchains++;
  }
  T.chunks.resize(n_chunks);
  T.streams.resize(call.size());
  T.zblocks.resize(n_zblocks);
  T.zitems.resize(n_zitems);
  uint32_t ci = 0;
  for (uint32_t si = 0; si < call.size(); si++) {
    const Use& u = call[si];
    StreamDesc& sd = T.streams[si];
    sd.first_chunk = ci;
    sd.n_chunks = (uint32_t)u.st->chunks.size();
    sd.len_idx = u.len_idx;
    sd.err_idx = u.err_idx;
    sd.base = u.plain;
    sd.framing_error = u.st->framing_error;
    sd.skip = u.st->skip;
    uint64_t slot = 0;
    for (auto& c : u.st->chunks) {
      ChunkDesc& cd = T.chunks[ci];
      cd.src = u.arena + u.st->arena_off + c.src_off;
      cd.dst = sd.base + slot;
      cd.scratch = chunk_rec_off[ci] != ~0ull ? S + chunk_rec_off[ci] : nullptr;
      cd.src_len = c.len;
      cd.dst_cap = c.plain_cap;
      cd.kind = c.original ? 0u : (uint32_t)u.st->compression;
      cd.stream = si;
      cd.out_len = 0;
      cd.status = 0;
      cd.first_item = chunk_first_item[ci];
      cd.n_items = 0;
      cd.diag = 0;
      cd.pad = 0;
      if (c.zparse >= 0) {
        const ZChunkParse& zp = u.st->zchunks[c.zparse];
        cd.n_items = (uint32_t)zp.items.size();
        if (zp.bad) cd.status = kCodecError;
        for (uint32_t k = 0; k < cd.n_items; k++) {
          const BlockPlan& bp = zitems[cd.first_item + k];
          const ZItemH& ih = *bp.item;
          ZItem& zi = T.zitems[cd.first_item + k];
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
            zi.nseq = ih.nseq;
            zi.zblock = bp.zblock;
            zi.seq_packed = seq_bytes == 8 ? 1u : 0u;
            ZBlock& zb = T.zblocks[bp.zblock];
            memset(&zb, 0, sizeof(zb));
            zb.src = cd.src;
            zb.lit_out = bp.lit_off != ~0ull ? S + bp.lit_off : nullptr;
            zb.seq_out = bp.seq_off != ~0ull ? reinterpret_cast<uint32_t*>(S + bp.seq_off) : nullptr;
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
          }
        }
      }
      slot += c.plain_cap;
      ci++;
    }
  }
  T.order = order_by_count_desc(n_chunks, [&](uint32_t c) -> int64_t {
    uint64_t ns = 0;
    const uint32_t f = chunk_first_item[c], e = c + 1 < n_chunks ? chunk_first_item[c + 1] : n_zitems;
    for (uint32_t k = f; k < e; k++) ns += zitems[k].item->nseq;
    return (int64_t)ns;
  });
  return T;
}

// ---- the code under test: the streams' own tables, merged and rebased ------------------------------------------------------------
static Tables merged_tables(const std::vector<Use>& call, uint8_t* S, uint64_t scratch0, uint32_t seq_bytes) {
  Tables T;
  std::vector<const StreamTables*> t;
  for (auto& u : call) t.push_back(&u.st->tables);
  TableCounts C;
  tables_count(t.data(), t.size(), C);
  Bump16 scratch{scratch0};
  std::vector<StreamUse> use(call.size());
  for (size_t k = 0; k < call.size(); k++) {
    const uint64_t need = t[k]->scratch_bytes(seq_bytes);
    use[k] = StreamUse{t[k], call[k].arena, call[k].plain, need ? S + scratch.take(need) : nullptr, call[k].len_idx, call[k].err_idx, call[k].st->framing_error, call[k].st->skip};
  }
  T.scratch_end = scratch.off;
  T.n_zchains = C.n_zchains;
  T.total_seq = C.total_seq;
  // (poisoned: every field must be written)
  T.chunks.resize(C.n_chunks);
  T.streams.resize(C.n_streams);
  T.zblocks.resize(C.n_zblocks);
  T.zitems.resize(C.n_zitems);
  T.order.assign(C.n_chunks, 0xdeadbeefu);
  if (C.n_chunks) memset(T.chunks.data(), 0xa5, C.n_chunks * sizeof(ChunkDesc));
  memset(T.streams.data(), 0xa5, C.n_streams * sizeof(StreamDesc));
  if (C.n_zblocks) memset(T.zblocks.data(), 0xa5, C.n_zblocks * sizeof(ZBlock));
  if (C.n_zitems) memset(T.zitems.data(), 0xa5, C.n_zitems * sizeof(ZItem));
  tables_fill(use.data(), C, seq_bytes == 8, T.chunks.data(), T.streams.data(), T.zblocks.data(), T.zitems.data(), T.order.data());
  return T;
}

static int g_bad = 0;
#define SAME(a, b, f)                                                                                       \
  do {                                                                                                      \
    if (!((a).f == (b).f)) {                                                                                \
      if (g_bad++ < 20) printf("  MISMATCH %s [%zu] .%s: %llu != %llu\n", what, (size_t)k, #f, (unsigned long long)(uintptr_t)(a).f, (unsigned long long)(uintptr_t)(b).f); \
    }                                                                                                       \
  } while (0)

static void compare(const char* what, const Tables& A, const Tables& B) {
  size_t k = 0;
  SAME(A, B, chunks.size());
  SAME(A, B, streams.size());
  SAME(A, B, zblocks.size());
  SAME(A, B, zitems.size());
  SAME(A, B, n_zchains);
  SAME(A, B, total_seq);
  SAME(A, B, scratch_end);
  if (g_bad) return;
  for (k = 0; k < A.chunks.size(); k++) {
    const ChunkDesc &a = A.chunks[k], &b = B.chunks[k];
    SAME(a, b, src); SAME(a, b, dst); SAME(a, b, scratch); SAME(a, b, src_len); SAME(a, b, dst_cap); SAME(a, b, kind); SAME(a, b, stream);
    SAME(a, b, out_len); SAME(a, b, status); SAME(a, b, first_item); SAME(a, b, n_items); SAME(a, b, diag); SAME(a, b, pad);
    SAME(A, B, order[k]);
  }
  for (k = 0; k < A.streams.size(); k++) {
    const StreamDesc &a = A.streams[k], &b = B.streams[k];
    SAME(a, b, first_chunk); SAME(a, b, n_chunks); SAME(a, b, len_idx); SAME(a, b, err_idx); SAME(a, b, base); SAME(a, b, framing_error); SAME(a, b, skip);
  }
  for (k = 0; k < A.zblocks.size(); k++) {
    const ZBlock &a = A.zblocks[k], &b = B.zblocks[k];
    SAME(a, b, src); SAME(a, b, lit_out); SAME(a, b, seq_out); SAME(a, b, chunk); SAME(a, b, content_off); SAME(a, b, content_end); SAME(a, b, lit_type);
    SAME(a, b, lit_streams); SAME(a, b, lit_hdr); SAME(a, b, lit_regen); SAME(a, b, lit_comp); SAME(a, b, nseq); SAME(a, b, seq_off); SAME(a, b, huf_off);
    SAME(a, b, huf_end); SAME(a, b, pad[0]); SAME(a, b, pad[1]);
    for (int w = 0; w < 3; w++) {
      SAME(a, b, tab_off[w]);
      SAME(a, b, tab_end[w]);
    }
    if (k && a.nseq > A.zblocks[k - 1].nseq && g_bad++ < 20) printf("  %s: block %zu has more sequences than the one before it\n", what, k);
  }
  for (k = 0; k < A.zitems.size(); k++) {
    const ZItem &a = A.zitems[k], &b = B.zitems[k];
    SAME(a, b, kind); SAME(a, b, flags); SAME(a, b, size); SAME(a, b, src_off); SAME(a, b, lit_kind); SAME(a, b, lit_off); SAME(a, b, litn); SAME(a, b, nseq);
    SAME(a, b, zblock); SAME(a, b, seq_packed); SAME(a, b, fcs); SAME(a, b, ck_off); SAME(a, b, pad);
  }
}

// ---- hand-made streams -------------------------------------------------------------------------------------------------------------
struct Blk {
  int kind;                  // 0 raw, 1 rle, 2 compressed
  uint32_t nseq = 0;
  int lit_type = 2;          // 0 raw literals, 1 one repeated byte, 2 Huffman with its tree, 3 treeless
  uint32_t lit_regen = 100;
  bool repeat_tables = false;  // the FSE tables are those of the block before
};
static std::mt19937 g_rng(12345);

// A Zstandard chunk of one frame made of `blocks`; returns its payload length
static uint32_t add_zchunk(Stream& st, const std::vector<Blk>& blocks, bool bad = false, bool size_known = true) {
  ZChunkParse zp;
  uint32_t pos = 6, plain = 0;
  int32_t huf = -1, tab = -1;
  for (auto& b : blocks) {
    ZItemH it;
    it.kind = (uint8_t)b.kind;
    it.off = pos + 3;
    if (b.kind == 0) {
      it.size = 50 + g_rng() % 1000;
      plain += it.size;
      pos = it.off + it.size;
    } else if (b.kind == 1) {
      it.size = 1 + g_rng() % 5000;
      it.rle_byte = (uint8_t)g_rng();
      plain += it.size;
      pos = it.off + 1;
    } else {
      it.lit_type = (uint8_t)b.lit_type;
      it.lit_streams = b.lit_type >= 2 && b.lit_regen > 255 ? 4 : 1;
      it.lit_hdr = 1 + g_rng() % 5;
      it.lit_regen = b.lit_regen;
      it.lit_comp = b.lit_type == 0 ? b.lit_regen : (b.lit_type == 1 ? 1 : b.lit_regen / 2 + 1);
      it.rle_byte = (uint8_t)g_rng();
      if (b.lit_type == 2) huf = (int32_t)zp.items.size();
      it.huf_def = b.lit_type == 3 ? huf : (b.lit_type == 2 ? huf : -1);
      if (b.lit_type == 3 && huf < 0) abort();  // (a case written wrongly)
      it.nseq = b.nseq;
      it.seq_off = it.off + it.lit_hdr + it.lit_comp + (b.nseq < 128 ? 1 : (b.nseq < 0x7f00 ? 2 : 3));
      it.size = it.seq_off - it.off + (b.nseq ? 1 + b.nseq * 2 : 0);
      if (b.nseq) {
        if (!b.repeat_tables || tab < 0) tab = (int32_t)zp.items.size();
        for (int w = 0; w < 3; w++) it.tab_def[w] = w == 1 && b.repeat_tables ? tab : (b.repeat_tables ? tab : (int32_t)zp.items.size());
      }
      plain += b.lit_regen + 3 * b.nseq;
      pos = it.off + it.size;
    }
    zp.items.push_back(it);
  }
  zp.items.front().flags |= 1;
  if (size_known) {
    zp.items.back().flags |= 2;
    zp.items.back().fcs = plain;
  }
  if (g_rng() % 2) {
    zp.items.back().flags |= 4;
    zp.items.back().ck_off = pos;
    pos += 4;
  }
  zp.size_known = size_known;
  zp.plain_size = plain;
  zp.bad = bad;
  if (bad) zp.items.clear();
  const uint64_t src_off = st.chunks.empty() ? 3 : st.chunks.back().src_off + st.chunks.back().len + 3;
  ChunkInfo ci{src_off, pos, 0, bad ? 0u : (size_known ? plain : 262144u), (int32_t)st.zchunks.size()};
  st.zchunks.push_back(zp);
  st.chunks.push_back(ci);
  return pos;
}
static void add_plain_chunk(Stream& st, uint32_t len, bool original, uint32_t plain_cap) {
  const uint64_t src_off = st.chunks.empty() ? 3 : st.chunks.back().src_off + st.chunks.back().len + 3;
  st.chunks.push_back(ChunkInfo{src_off, len, original ? 1u : 0u, original ? len : plain_cap, -1});
}
static void finish(std::vector<Stream>& stripe) {  // arena offsets, tables: what staging does
  uint64_t off = 0;
  for (auto& st : stripe) {
    st.arena_off = off;
    off += (st.chunks.empty() ? 0 : st.chunks.back().src_off + st.chunks.back().len) + 32;
    off = (off + 255) & ~255ull;
    build_stream_tables(st.chunks, st.zchunks, st.compression, st.arena_off, kCodecError, st.tables);
  }
}

static std::string snapshot(const StreamTables& t) {  // the tables' bytes: a call must leave them alone
  std::string s;
  auto add = [&](const void* p, size_t n) { s.append(reinterpret_cast<const char*>(p), n); };
  add(t.chunks.data(), t.chunks.size() * sizeof(ChunkDesc));
  add(t.items.data(), t.items.size() * sizeof(ZItem));
  add(t.zblocks.data(), t.zblocks.size() * sizeof(ZBlock));
  add(t.zb_item.data(), t.zb_item.size() * 4);
  add(t.zb_seq_before.data(), t.zb_seq_before.size() * 8);
  add(t.zb_hist.data(), t.zb_hist.size() * sizeof(t.zb_hist[0]));
  add(t.chunk_order.data(), t.chunk_order.size() * 4);
  add(t.chunk_hist.data(), t.chunk_hist.size() * sizeof(t.chunk_hist[0]));
  return s;
}

static int g_cases = 0;
// A call over the streams picked from the stripes, in that order; both sequence sizes
static void run(const char* what, const std::vector<const std::vector<Stream>*>& stripes, const std::vector<std::pair<int, int>>& pick = {}) {
  uint8_t* const S = reinterpret_cast<uint8_t*>((uintptr_t)0x7000000000ull);  // (never dereferenced: the tables only hold addresses)
  std::vector<Use> call;
  std::vector<std::string> before;
  auto add = [&](int s, int k) {
    const Stream& st = (*stripes[s])[k];
    uint64_t cap = 0;
    for (auto& c : st.chunks) cap += c.plain_cap;
    const uint32_t n = (uint32_t)call.size();
    call.push_back(Use{&st, reinterpret_cast<const uint8_t*>((uintptr_t)0x1000000000ull * (s + 1)), reinterpret_cast<uint8_t*>((uintptr_t)0x5000000000ull + 0x10000000ull * n + 256 * (g_rng() % 64)), 2 * n + 7, 2 * n + 8});
    before.push_back(snapshot(st.tables));
    (void)cap;
  };
  if (pick.empty()) {
    for (size_t s = 0; s < stripes.size(); s++)
      for (size_t k = 0; k < stripes[s]->size(); k++) add((int)s, (int)k);
  } else {
    for (auto& p : pick) add(p.first, p.second);
  }
  const int bad0 = g_bad;
  for (uint32_t seq_bytes : {12u, 8u}) {
    const uint64_t scratch0 = 256 * (1 + g_rng() % 100);
    const Tables want = reference_tables(call, S, scratch0, seq_bytes), got = merged_tables(call, S, scratch0, seq_bytes);
    compare(what, got, want);
  }
  for (size_t k = 0; k < call.size(); k++)
    if (snapshot(call[k].st->tables) != before[k]) printf("  %s: the tables of stream %zu were changed by a call\n", what, k), g_bad++;
  size_t blocks = 0, chunks = 0;
  for (auto& u : call) blocks += u.st->tables.zblocks.size(), chunks += u.st->chunks.size();
  printf("%s: %zu streams, %zu chunks, %zu blocks: %s\n", what, call.size(), chunks, blocks, g_bad == bad0 ? "same" : "DIFFERENT");
  g_cases++;
}

static std::vector<Stream> zstd_stripe(int n_streams, const std::vector<uint32_t>& counts, bool odd_blocks) {
  std::vector<Stream> stripe(n_streams);
  size_t at = 0;
  for (auto& st : stripe) {
    const int n_chunks = 1 + (int)(g_rng() % 3);
    for (int c = 0; c < n_chunks; c++) {
      std::vector<Blk> blocks;
      const int nb = 1 + (int)(g_rng() % 4);
      for (int b = 0; b < nb; b++) {
        Blk k{2, counts[at++ % counts.size()], b == 0 ? 2 : (int)(2 + g_rng() % 2), (uint32_t)(1 + g_rng() % 70000), b > 0 && g_rng() % 2 == 0};
        blocks.push_back(k);
        if (odd_blocks && g_rng() % 3 == 0) blocks.push_back(Blk{(int)(g_rng() % 2)});
      }
      add_zchunk(st, blocks);
    }
  }
  finish(stripe);
  return stripe;
}

int main() {
  (void)&zstd_parse_chunk;  // (the parser is not what is checked here: the cases hand the builder parsed blocks)
  // one stripe
  const std::vector<Stream> one = zstd_stripe(5, {7, 30000, 512, 3, 129, 40000, 1, 127, 128, 5000}, true);
  run("one stripe", {&one});
  // three stripes with equal sequence counts across stripes: the order within a count is the order in the call
  const std::vector<Stream> e1 = zstd_stripe(4, {100, 200, 100, 300, 200}, false), e2 = zstd_stripe(3, {200, 100, 300}, false), e3 = zstd_stripe(4, {300, 300, 100, 200}, false);
  run("three stripes, equal counts", {&e1, &e2, &e3});
  run("three stripes, equal counts, other order", {&e3, &e1, &e2});
  // a stripe without a Zstandard block between two that have some
  std::vector<Stream> none(3);
  add_plain_chunk(none[0], 1000, true, 0);
  add_plain_chunk(none[0], 17, true, 0);
  add_zchunk(none[1], {Blk{0}, Blk{1}, Blk{0}});  // (raw and RLE blocks only)
  add_plain_chunk(none[2], 1, true, 0);
  finish(none);
  run("no compressed block in the middle stripe", {&e1, &none, &e2});
  run("only a stripe without compressed blocks", {&none});
  // a chunk stored "original" among compressed ones; a block without sequences; raw and RLE literals; a treeless block; a chunk
  // whose headers did not parse; a frame that does not state its size
  std::vector<Stream> mix(3);
  add_zchunk(mix[0], {Blk{2, 900, 2, 4000}, Blk{2, 0, 2, 70000}, Blk{2, 900, 3, 300, true}});
  add_plain_chunk(mix[0], 4321, true, 0);
  add_zchunk(mix[0], {Blk{2, 0, 0, 55}, Blk{2, 12, 1, 131072}, Blk{1}, Blk{2, 0, 1, 9}});
  add_zchunk(mix[1], {Blk{2, 5, 2, 10}}, true);
  add_zchunk(mix[1], {Blk{2, 77, 0, 1000}, Blk{0}}, false, false);
  add_plain_chunk(mix[2], 99, true, 0);
  add_zchunk(mix[2], {Blk{2, 1, 2, 1}});
  mix[2].framing_error = 1;
  finish(mix);
  run("original chunk, nseq 0, raw / RLE literals, bad chunk, unknown size", {&mix});
  run("... between two stripes", {&e2, &mix, &one});
  // a stripe staged under a row selection: the chunk lists start inside the streams and the decoders skip into the first chunk;
  // and a call that takes some of a stripe's streams only (a column lane), in another order than they were staged
  std::vector<Stream> sub = zstd_stripe(4, {64, 64, 2000, 9, 64}, true);
  for (auto& st : sub) {
    st.chunks.erase(st.chunks.begin(), st.chunks.begin() + (st.chunks.size() > 1 ? 1 : 0));  // (zparse keeps pointing at the chunk's own parse)
    st.skip = 1 + g_rng() % 500;
  }
  finish(sub);
  run("chunk lists that are subsets", {&sub});
  run("some streams of each stripe", {&one, &sub, &e1}, {{0, 4}, {0, 1}, {1, 2}, {2, 0}, {2, 3}, {1, 0}});
  run("the same stream alone", {&one}, {{0, 1}});
  run("the same stream with another partner", {&one, &e3}, {{1, 2}, {0, 1}});
  // chunks whose sequences exceed 2^18 share the top bucket in index order
  std::vector<Stream> big(2);
  add_zchunk(big[0], std::vector<Blk>(9, Blk{2, 30000, 2, 10}));
  add_zchunk(big[0], std::vector<Blk>(10, Blk{2, 30000, 2, 10}));
  add_zchunk(big[1], {Blk{2, 98047, 2, 10}});
  add_zchunk(big[1], std::vector<Blk>(11, Blk{2, 30000, 2, 10}));
  finish(big);
  run("chunks above the top bucket", {&big, &e1});
  // Snappy, LZ4 and zlib: the record scratch of a chunk
  for (int comp : {ORCGPU_COMP_SNAPPY, ORCGPU_COMP_LZ4, ORCGPU_COMP_ZLIB}) {
    std::vector<Stream> rec(2);
    for (auto& st : rec) {
      st.compression = comp;
      add_plain_chunk(st, 1 + g_rng() % 100000, false, 262144);
      add_plain_chunk(st, 5, true, 0);
      add_plain_chunk(st, 2, false, 7);
      add_plain_chunk(st, 262144, false, 262144);
    }
    finish(rec);
    for (auto& st : rec) {
      uint64_t want = 0;
      for (auto& c : st.chunks) {
        want = (want + 15) & ~15ull;
        if (c.original) continue;
        if (comp == ORCGPU_COMP_SNAPPY) want += 8ull * (c.len / 2 + 2);
        if (comp == ORCGPU_COMP_LZ4) want += 8ull * (2 * (c.len / 3 + 1) + 2);
        if (comp == ORCGPU_COMP_ZLIB) want += (((uint64_t)c.plain_cap + 16 + 15) & ~15ull) + 12ull * (c.plain_cap / 3 + 2) + 16;
      }
      if (st.tables.scratch_bytes(12) != want || st.tables.scratch_bytes(8) != want) printf("  record scratch of codec %d: %llu, not %llu\n", comp, (unsigned long long)st.tables.scratch_bytes(12), (unsigned long long)want), g_bad++;
    }
    run(comp == ORCGPU_COMP_SNAPPY ? "snappy" : (comp == ORCGPU_COMP_LZ4 ? "lz4" : "zlib"), {&rec});
  }
  // the sequence scratch: 12 bytes a sequence for three arrays, 8 for packed records, either with ((nseq + 3) & ~3) sequences + 16
  {
    std::vector<Stream> s(1);
    add_zchunk(s[0], {Blk{2, 5, 0, 10}, Blk{2, 8, 1, 10}});
    finish(s);
    const uint64_t w12 = 12 * 8 + 16 + 12 * 8 + 16, w8 = 8 * 8 + 16 + 8 * 8 + 16;
    if (s[0].tables.scratch_bytes(12) != w12 || s[0].tables.scratch_bytes(8) != w8) printf("  sequence scratch: %llu / %llu\n", (unsigned long long)s[0].tables.scratch_bytes(12), (unsigned long long)s[0].tables.scratch_bytes(8)), g_bad++;
  }
  // one stream of a stripe, and an empty call
  run("one stream of five", {&one}, {{0, 0}});
  {
    TableCounts C;
    tables_count(nullptr, 0, C);
    tables_fill(nullptr, C, false, nullptr, nullptr, nullptr, nullptr, nullptr);
  }
  printf("checked %d calls, %d mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
