// device/writer_kinds.h -- what the stripe writer's host code (orcgpu_writer_host.inc) and its row index kernels
// (device/col_stats.hip) share: the column kinds and a row group's statistics record.  Plain C++: no HIP, no kernels.
#pragma once
#include <cstdint>

// How a column is held on the device and which streams it writes (WrCol::kind, IxCol::kind).  The values are a device ABI:
// the kernels receive them as int32_t.
enum WrKind : int32_t {
  WR_INT = 0,        // Integer RLE v2 (signed)
  WR_BYTE = 1,       // byte RLE
  WR_FLOAT = 2,      // raw floats
  WR_BOOL = 3,       // Boolean: bits over byte RLE
  WR_STRING = 4,     // strings: bytes + unsigned RLE v2 lengths (or a dictionary)
  WR_TIMESTAMP = 5,  // seconds + nanosecond codes, RLE v2
  WR_DECIMAL = 6,    // Decimal128: varint bytes + the scale, signed RLE v2
  WR_STRUCT = 7,     // PRESENT alone
  WR_LIST = 8,       // List / Map: the valid rows' lengths, unsigned RLE v2, in the offsets' width
};

#define IX_STR_KEEP 1025u  // bytes of a string minimum / maximum the host receives (a bound is cut at 1024)

struct IxRec {  // one job's statistics, 128 bytes (the host reads them as they are)
  uint64_t count, bytes, trues;
  union {  // integers: the minimum; floats: the sum of the values of magnitude >= 2^960, scaled by 2^-64 (a double-double)
    int64_t imin;
    double dbig;
  };
  union {
    int64_t imax;
    double dbig_lo;
  };
  uint64_t sum_lo;
  int64_t sum_hi;  // integer sum: sum_hi:sum_lo, two's complement
  double dmin, dmax, dsum, dsum_lo;
  uint64_t smin_at, smax_at;  // strings: offsets of the minimum / maximum in the column's bytes
  uint64_t side;              // ... and of their copies in the side buffer (minimum, then maximum)
  uint32_t smin_len, smax_len;
  uint32_t has_null, has_nan;
  // Timestamp: imin / imax the minimum's / maximum's second, sum_lo / sum_hi their nanoseconds.
  // Decimal128: imin:imax the minimum (low, high word), smin_at:smax_at the maximum, sum_lo:sum_hi:trues the sum in 192 bits.
};
static_assert(sizeof(IxRec) == 128, "IxRec is read by the host as 128 bytes");
