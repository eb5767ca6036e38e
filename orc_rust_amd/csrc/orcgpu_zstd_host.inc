// orcgpu_zstd_host.inc -- host-side parse of the Zstandard frame and block headers of one ORC chunk
// (RFC 8878 3.1.1: frame header, block headers, literals section header, Number_of_Sequences), done
// while the stripe is staged and the bytes are in host memory anyway -- like the 3-byte ORC chunk
// headers (SURVEY 2 K0).  It is what lets the device decode every Compressed_Block independently
// (zstd_entropy.h) and gives a Zstandard chunk an exact slot in the plain buffer whenever its frames
// state their content size.  Everything it rejects the oracle's decoder rejects too
// (oracle/oo_codecs.c: oo_zstd_frame, z_block, z_literals).
namespace {

struct ZItemH {
  uint8_t kind = 0;          // 0 raw, 1 rle, 2 compressed
  uint8_t flags = 0;         // 1 first block of a frame, 2 last block of a frame with a content size, 4 last block of a frame with a content checksum
  uint32_t off = 0;          // block content inside the chunk payload
  uint32_t size = 0;         // raw / rle: regenerated size; compressed: size of the content
  uint8_t rle_byte = 0;
  // compressed blocks
  uint8_t lit_type = 0, lit_streams = 1;
  uint32_t lit_hdr = 0, lit_regen = 0, lit_comp = 0;
  uint32_t nseq = 0, seq_off = 0;
  int32_t huf_def = -1;      // item whose literals section holds the Huffman tree this block uses
  int32_t tab_def[3] = {-1, -1, -1};  // item whose sequences section describes the LL / OF / ML table this block uses
  uint64_t fcs = 0;
  uint32_t block_max = 0;    // compressed: Block_Maximum_Size of its frame, the most it may regenerate
  uint32_t ck_off = 0;       // flags & 4: where the checksum's four bytes lie in the chunk payload
};

struct ZChunkParse {
  bool bad = false;
  bool size_known = true;    // every frame states its content size
  uint64_t plain_size = 0;   // sum of the content sizes
  std::vector<ZItemH> items;
};

void zstd_parse_chunk(const uint8_t* src, uint32_t n, ZChunkParse& out) {
  uint32_t pos = 0;
  auto fail = [&] { out.bad = true; };
  while (pos < n) {
    if (pos + 4 > n) return fail();
    const uint32_t magic = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8) | ((uint32_t)src[pos + 2] << 16) | ((uint32_t)src[pos + 3] << 24);
    if ((magic & 0xfffffff0u) == 0x184d2a50u) {  // skippable frame
      if (pos + 8 > n) return fail();
      const uint32_t sz = (uint32_t)src[pos + 4] | ((uint32_t)src[pos + 5] << 8) | ((uint32_t)src[pos + 6] << 16) | ((uint32_t)src[pos + 7] << 24);
      if ((uint64_t)pos + 8 + sz > n) return fail();
      pos += 8 + sz;
      continue;
    }
    if (magic != 0xfd2fb528u) return fail();
    pos += 4;
    if (pos >= n) return fail();
    const uint32_t fhd = src[pos++];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, has_ck = (fhd >> 2) & 1, did_flag = fhd & 3;
    if (fhd & 0x08) return fail();
    uint64_t window = 0;
    if (!single) {
      if (pos >= n) return fail();
      // window descriptor: the whole frame is decoded into the chunk's slot; the window only bounds the blocks' sizes
      const uint32_t wd = src[pos++];
      const uint64_t base = 1ull << (10 + (wd >> 3));
      window = base + (base >> 3) * (wd & 7);
    }
    const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
    if (did_bytes) {
      if (pos + did_bytes > n) return fail();
      uint32_t did = 0;
      for (uint32_t i = 0; i < did_bytes; i++) did |= (uint32_t)src[pos + i] << (8 * i);
      pos += did_bytes;
      if (did) return fail();  // dictionaries are not used by ORC
    }
    const uint32_t fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : (fcs_flag == 1 ? 2 : (fcs_flag == 2 ? 4 : 8));
    uint64_t fcs = 0;
    if (pos + fcs_bytes > n) return fail();
    for (uint32_t i = 0; i < fcs_bytes; i++) fcs |= (uint64_t)src[pos + i] << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    pos += fcs_bytes;
    if (single) window = fcs;
    // Block_Maximum_Size (RFC 8878 3.1.1.2.4): the smaller of the window and 128 KiB, for what a block of any type holds and regenerates
    const uint32_t block_max = (uint32_t)std::min<uint64_t>(window, 128 * 1024);
    if (fcs_bytes) out.plain_size += fcs;
    else out.size_known = false;
    const size_t first = out.items.size();
    int32_t huf_def = -1, tab_def[3] = {-1, -1, -1};
    uint32_t last;
    do {
      if (pos + 3 > n) return fail();
      const uint32_t bh = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8) | ((uint32_t)src[pos + 2] << 16);
      pos += 3;
      last = bh & 1;
      const uint32_t bt = (bh >> 1) & 3, bs = bh >> 3;
      if (bs > block_max) return fail();  // (Raw and RLE blocks too: their Block_Size is what they regenerate)
      ZItemH it;
      it.off = pos;
      if (bt == 0) {
        if ((uint64_t)pos + bs > n) return fail();
        it.kind = 0;
        it.size = bs;
        pos += bs;
      } else if (bt == 1) {
        if (pos + 1 > n) return fail();
        it.kind = 1;
        it.size = bs;
        it.rle_byte = src[pos];
        pos += 1;
      } else if (bt == 2) {
        if ((uint64_t)pos + bs > n) return fail();
        it.kind = 2;
        it.size = bs;
        it.block_max = block_max;
        const uint8_t* p = src + pos;
        if (bs < 1) return fail();
        const uint32_t type = p[0] & 3, sf = (p[0] >> 2) & 3;
        uint32_t regen, comp = 0, hdr, streams = 1;
        if (type < 2) {
          if (sf == 0 || sf == 2) {
            regen = p[0] >> 3;
            hdr = 1;
          } else if (sf == 1) {
            if (bs < 2) return fail();
            regen = (p[0] >> 4) | ((uint32_t)p[1] << 4);
            hdr = 2;
          } else {
            if (bs < 3) return fail();
            regen = (p[0] >> 4) | ((uint32_t)p[1] << 4) | ((uint32_t)p[2] << 12);
            hdr = 3;
          }
          if (regen > 128 * 1024) return fail();
          if (type == 0) {
            if ((uint64_t)hdr + regen > bs) return fail();
            comp = regen;
          } else {
            if (hdr + 1 > bs) return fail();
            comp = 1;
            it.rle_byte = p[hdr];
          }
        } else {
          if (sf == 0 || sf == 1) {
            if (bs < 3) return fail();
            const uint32_t v = p[0] | (p[1] << 8) | (p[2] << 16);
            regen = (v >> 4) & 0x3ff;
            comp = (v >> 14) & 0x3ff;
            hdr = 3;
            streams = sf == 0 ? 1 : 4;
          } else if (sf == 2) {
            if (bs < 4) return fail();
            const uint32_t v = p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24);
            regen = (v >> 4) & 0x3fff;
            comp = (v >> 18) & 0x3fff;
            hdr = 4;
            streams = 4;
          } else {
            if (bs < 5) return fail();
            const uint64_t v = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24) | ((uint64_t)p[4] << 32);
            regen = (uint32_t)((v >> 4) & 0x3ffff);
            comp = (uint32_t)((v >> 22) & 0x3ffff);
            hdr = 5;
            streams = 4;
          }
          if (regen > 128 * 1024 || (uint64_t)hdr + comp > bs) return fail();
          if (type == 2) huf_def = (int32_t)out.items.size();
          else if (huf_def < 0) return fail();  // Treeless literals without a table in this frame
        }
        it.lit_type = (uint8_t)type;
        it.lit_streams = (uint8_t)streams;
        it.lit_hdr = hdr;
        it.lit_regen = regen;
        it.lit_comp = comp;
        it.huf_def = huf_def;
        // Number_of_Sequences
        uint32_t q = hdr + comp;
        if (q + 1 > bs) return fail();
        uint32_t nseq;
        if (p[q] < 128) {
          nseq = p[q];
          q += 1;
        } else if (p[q] < 255) {
          if (q + 2 > bs) return fail();
          nseq = ((uint32_t)(p[q] - 128) << 8) + p[q + 1];
          q += 2;
        } else {
          if (q + 3 > bs) return fail();
          nseq = (uint32_t)p[q + 1] + ((uint32_t)p[q + 2] << 8) + 0x7f00;
          q += 3;
        }
        it.nseq = nseq;
        it.seq_off = pos + q;
        if (nseq) {
          if (q + 1 > bs) return fail();
          const uint32_t modes = p[q];
          if (modes & 3) return fail();
          for (int w = 0; w < 3; w++) {
            const uint32_t mode = (modes >> (6 - 2 * w)) & 3;
            if (mode != 3) tab_def[w] = (int32_t)out.items.size();
            else if (tab_def[w] < 0) return fail();  // Repeat_Mode without a table in this frame
            it.tab_def[w] = tab_def[w];
          }
        }
        pos += bs;
      } else {
        return fail();
      }
      out.items.push_back(it);
    } while (!last);
    out.items[first].flags |= 1;
    if (fcs_bytes) {
      out.items.back().flags |= 2;
      out.items.back().fcs = fcs;
    }
    if (has_ck) {
      // XXH64 content checksum (low 32 bits): verified by the execution kernel behind the frame's last block, as libzstd does
      if (pos + 4 > n) return fail();
      out.items.back().flags |= 4;
      out.items.back().ck_off = pos;
      pos += 4;
    }
  }
}

}  // namespace
