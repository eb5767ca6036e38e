/*
 * orcgpu.h -- C ABI of the MI355X-native ORC stripe decoder (liborcgpu.so).
 *
 * Drop-in boundary.  In datafusion-contrib/orc-rust the stripe -> Arrow hot path sits behind a
 * Rust trait-object seam, not an FFI:
 *     NaiveStripeDecoder::new_with_selection(stripe, schema_ref, batch_size, row_selection)
 *         src/array_decoder/mod.rs:570-594, installed at src/arrow_reader.rs:310-316
 *     trait ArrayBatchDecoder::next_batch(batch_size, parent_present) -> ArrayRef
 *         src/array_decoder/mod.rs:61-85, built by array_decoder_factory  :390-511
 * The inputs at that seam are `Stripe { columns, stream_map: HashMap<(u32, Kind), Bytes>,
 * compression, number_of_rows, tz }` (src/stripe.rs:119-125, :311-316).  This header is what a
 * Rust shim implementing `Iterator<Item = Result<RecordBatch>>` binds instead of building the
 * CPU decoders (see INTEGRATION.md for the `extern "C"` block and the arrow::ffi import).
 *
 * Everything below is plain C: pointers, sizes and POD structs; no C++/torch types.
 * Threading: a context is thread-compatible (one thread at a time, may migrate), like
 * `ArrayBatchDecoder: Send` (array_decoder/mod.rs:61) -- with one exception that pipelines need: orcgpu_stage_stripe may run
 * in one thread while another one decodes / fetches / frees on the same context.
 */
#ifndef ORCGPU_H
#define ORCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: 1:1 with the OrcError variants the path raises (src/error.rs:31-174) ---- */
enum {
  ORCGPU_OK = 0,
  ORCGPU_IO_ERROR = 1,          /* IoError (short read / unexpected end of stream)          */
  ORCGPU_OUT_OF_SPEC = 2,       /* OutOfSpec { msg }                                        */
  ORCGPU_VARINT_TOO_LARGE = 3,  /* VarintTooLarge                                           */
  ORCGPU_DECODE_TIMESTAMP = 4,  /* DecodeTimestamp { seconds, nanoseconds, to_time_unit }   */
  ORCGPU_OFFSET_OVERFLOW = 5,   /* OffsetOverflow { total_length, max_size, batch_size }    */
  ORCGPU_MISMATCHED_SCHEMA = 6, /* MismatchedSchema { orc_type, arrow_type }                */
  ORCGPU_UNSUPPORTED = 7,       /* UnsupportedTypeVariant { msg }                           */
  ORCGPU_ARROW = 8,             /* Arrow (UTF-8 validation, dictionary key, offsets)        */
  ORCGPU_BUILD_DECODER = 9,     /* Build{Zstd,Snappy,Lz4}Decoder / inflate failure          */
  ORCGPU_UNEXPECTED = 10,       /* Unexpected { msg }                                       */
  ORCGPU_HIP_ERROR = 100,       /* HIP runtime failure (no device, out of memory, ...)      */
  ORCGPU_INVALID_ARGUMENT = 101,
  ORCGPU_END_OF_FILE = 110      /* not an error: orcgpu_reader_next_batch has handed out every batch (Iterator::next -> None) */
};

/* proto CompressionKind (format/orc_proto.proto:383-390) */
enum { ORCGPU_COMP_NONE = 0, ORCGPU_COMP_ZLIB = 1, ORCGPU_COMP_SNAPPY = 2, ORCGPU_COMP_LZO = 3, ORCGPU_COMP_LZ4 = 4, ORCGPU_COMP_ZSTD = 5 };

/* proto Type.Kind (format/orc_proto.proto:199-228; src/schema.rs:241-320) */
enum {
  ORCGPU_T_BOOLEAN = 0, ORCGPU_T_BYTE = 1, ORCGPU_T_SHORT = 2, ORCGPU_T_INT = 3, ORCGPU_T_LONG = 4, ORCGPU_T_FLOAT = 5,
  ORCGPU_T_DOUBLE = 6, ORCGPU_T_STRING = 7, ORCGPU_T_BINARY = 8, ORCGPU_T_TIMESTAMP = 9, ORCGPU_T_LIST = 10,
  ORCGPU_T_MAP = 11, ORCGPU_T_STRUCT = 12, ORCGPU_T_UNION = 13, ORCGPU_T_DECIMAL = 14, ORCGPU_T_DATE = 15,
  ORCGPU_T_VARCHAR = 16, ORCGPU_T_CHAR = 17, ORCGPU_T_TIMESTAMP_INSTANT = 18
};

/* proto Stream.Kind (format/orc_proto.proto:125-143) */
enum { ORCGPU_S_PRESENT = 0, ORCGPU_S_DATA = 1, ORCGPU_S_LENGTH = 2, ORCGPU_S_DICTIONARY_DATA = 3, ORCGPU_S_DICTIONARY_COUNT = 4,
       ORCGPU_S_SECONDARY = 5, ORCGPU_S_ROW_INDEX = 6, ORCGPU_S_BLOOM_FILTER = 7, ORCGPU_S_BLOOM_FILTER_UTF8 = 8 };

/* proto ColumnEncoding.Kind (format/orc_proto.proto:150-155; src/column.rs:47-59) */
enum { ORCGPU_ENC_DIRECT = 0, ORCGPU_ENC_DICTIONARY = 1, ORCGPU_ENC_DIRECT_V2 = 2, ORCGPU_ENC_DICTIONARY_V2 = 3 };

/* Arrow target of a column = the `hinted_arrow_type` of array_decoder_factory (mod.rs:390-394).
 * 0 picks the default mapping of src/schema.rs:503-579. */
enum {
  ORCGPU_ARROW_DEFAULT = 0,
  /* the default mapping at another time unit (with_timestamp_precision): Timestamp -> Timestamp(unit), TimestampInstant -> Timestamp(unit, "UTC") */
  ORCGPU_ARROW_TIMESTAMP_S = 1, ORCGPU_ARROW_TIMESTAMP_MS = 2, ORCGPU_ARROW_TIMESTAMP_US = 3, ORCGPU_ARROW_TIMESTAMP_NS = 4,
  /* an explicit Arrow type (with_schema): the pairs array_decoder_factory accepts decode, every other pair is
   * ORCGPU_MISMATCHED_SCHEMA (mod.rs:390-511, timestamp.rs:149-232) */
  ORCGPU_ARROW_BOOLEAN = 10, ORCGPU_ARROW_INT8 = 11, ORCGPU_ARROW_INT16 = 12, ORCGPU_ARROW_INT32 = 13, ORCGPU_ARROW_INT64 = 14,
  ORCGPU_ARROW_FLOAT32 = 15, ORCGPU_ARROW_FLOAT64 = 16, ORCGPU_ARROW_UTF8 = 17, ORCGPU_ARROW_BINARY = 18, ORCGPU_ARROW_DATE32 = 19,
  ORCGPU_ARROW_DECIMAL128 = 20,  /* precision / scale in arrow_precision / arrow_scale; (38, 9) is also the wide target of timestamps */
  ORCGPU_ARROW_TIMESTAMP_S_UTC = 21, ORCGPU_ARROW_TIMESTAMP_MS_UTC = 22, ORCGPU_ARROW_TIMESTAMP_US_UTC = 23, ORCGPU_ARROW_TIMESTAMP_NS_UTC = 24,
  ORCGPU_ARROW_LARGE_UTF8 = 25, ORCGPU_ARROW_LARGE_BINARY = 26,  /* (the encoder's inputs only: i64 offsets) */
  /* Dictionary(Int32, Utf8) for a STRING / VARCHAR / CHAR column, at the root or as a Struct field: int32 keys per row and one
   * dictionary per stripe instead of Utf8 (orcgpu_dictionary_view below).  Beyond the reference, which casts its DictionaryArray
   * back to a StringArray (array_decoder/string.rs:216-219).  Any other ORC type with it: ORCGPU_MISMATCHED_SCHEMA */
  ORCGPU_ARROW_DICTIONARY_UTF8 = 27,
  ORCGPU_ARROW_TIMESTAMP_S_NOTZ = 31, ORCGPU_ARROW_TIMESTAMP_MS_NOTZ = 32, ORCGPU_ARROW_TIMESTAMP_US_NOTZ = 33, ORCGPU_ARROW_TIMESTAMP_NS_NOTZ = 34,
  ORCGPU_ARROW_TIMESTAMP_OTHER_TZ = 35,  /* Timestamp(_, Some(tz)) with tz != "UTC": UnsupportedTypeVariant for TimestampInstant */
  /* nested targets (array_decoder/mod.rs:464-505): the hint of a Struct / List / Map / Union column; its children carry theirs */
  ORCGPU_ARROW_STRUCT = 40, ORCGPU_ARROW_LIST = 41, ORCGPU_ARROW_MAP = 42, ORCGPU_ARROW_UNION = 43,
  ORCGPU_ARROW_MAP_SORTED = 44,  /* Map with keys_sorted: UnsupportedTypeVariant "Sorted map" */
  ORCGPU_ARROW_OTHER = 99        /* any Arrow type the path has no decoder for */
};

typedef struct orcgpu_ctx orcgpu_ctx;          /* one GPU, one HIP stream, reusable workspace */
typedef struct orcgpu_staged orcgpu_staged;    /* stripe streams resident in HBM              */
typedef struct orcgpu_result orcgpu_result;    /* decoded Arrow buffers resident in HBM       */

typedef struct {
  uint64_t workspace_bytes;  /* initial HBM workspace (0 = grow on demand)  */
  uint32_t flags;            /* reserved, 0                                 */
} orcgpu_opts;

/* One entry of Stripe.stream_map (src/stripe.rs:311-316): raw, possibly compressed bytes. */
/* Where a row group starts in a stream: what a RowIndexEntry holds for it (row_index.rs:42-50; orcgpu_index_entry below deals
 * an entry's positions out to the column's streams). */
typedef struct {
  uint64_t chunk_offset;  /* where, in the stream's bytes, the entry's chunk header is (uncompressed file: the byte itself) */
  uint32_t skip_bytes;    /* bytes into the decompressed chunk (uncompressed: 0)                                         */
  uint32_t skip_values;   /* run-length streams: values (bit streams: bytes) of the run there already consumed            */
  uint32_t skip_bits;     /* bit streams: bits of that byte consumed                                                     */
} orcgpu_stream_entry;

typedef struct {
  uint32_t column_id;
  int32_t kind;        /* ORCGPU_S_* */
  const uint8_t* ptr;  /* HOST pointer (pageable or pinned) */
  uint64_t len;
  /* Entry point (0, 0: the stream is given from its start).  A stream may be given from a row group on: `ptr` then starts at
   * the chunk header (compressed file) or at the byte (uncompressed file) a ROW_INDEX position names, and the decoder of the
   * stream starts `skip_bytes` into the (decompressed) bytes and drops the first `skip_values` values it decodes there -- the
   * three numbers a RowIndexEntry holds per stream (row_index.rs:42-50; orcgpu_index_entry splits an entry's positions by
   * stream).  Dictionary streams (DICTIONARY_DATA, the LENGTH stream of a dictionary) are always given whole.  The bytes may
   * reach beyond what the rows need: what lies behind the values the stripe's rows consume is not looked at. */
  uint32_t skip_bytes;
  uint32_t skip_values; /* PRESENT / Boolean DATA: in bytes of the bit stream; the bits of the byte there already consumed: skip_bits below */
  /* Optional (NULL, 0: none): where the stripe's later row groups start in this stream, in stream order, chunk_offset counted
   * from `ptr` -- the ROW_INDEX positions of the stream.  Run-length streams use them as verified run starts: one lane per
   * row group follows the run headers from its entry to the next (some tens of dependent steps instead of the whole stream's),
   * which gives every 512-byte block of the stream its first header without the search the decoder otherwise makes for
   * them.  Only a hint: entries that do not lie on the stream's run chain are noticed and ignored. */
  const orcgpu_stream_entry* entries;
  uint32_t n_entries;
  uint32_t skip_bits;   /* PRESENT / Boolean DATA entered at a row group: bits (0..7) of the first byte that belong to the rows before */
} orcgpu_stream;

/* One projected leaf column: what Column / DataType / ColumnEncoding carry (src/column.rs:24-59). */
typedef struct {
  uint32_t column_id;
  int32_t orc_type;          /* ORCGPU_T_*                                   */
  int32_t encoding;          /* ORCGPU_ENC_*  (rle version = column.rs:52-59) */
  uint32_t dictionary_size;  /* column.rs:40-45                              */
  uint32_t precision, scale; /* DECIMAL                                      */
  int32_t arrow_target;      /* ORCGPU_ARROW_*                               */
  uint32_t arrow_precision, arrow_scale; /* ORCGPU_ARROW_DECIMAL128           */
  uint32_t parent;           /* 0: a root column; else 1 + the index in `columns` of the STRUCT this column is a field of
                              * (Column::children, column.rs; parents come before their children).  A STRUCT column is
                              * given with orc_type ORCGPU_T_STRUCT: it decodes to a validity bitmap, and its fields' validity
                              * is theirs merged with it (array_decoder/struct_decoder.rs:58-78, mod.rs:216-252) */
} orcgpu_column;

typedef struct {
  uint64_t n_rows;           /* Stripe.number_of_rows                                              */
  int32_t compression;       /* ORCGPU_COMP_* (Compression::from_proto, src/compression.rs:52-83)  */
  uint64_t block_size;       /* max_decompressed_block_size, 0 = 262144 (compression.rs:31).  What a chunk of a conforming writer
                              * expands to at most, and what lz4_flex enforces (compression.rs:185-195).  flate2, lzokay and the
                              * zstd crate grow their output instead: a chunk of theirs that does not fit is decoded again with
                              * room for max(block_size, 4 MiB), beyond which it is ORCGPU_BUILD_DECODER */
  int64_t ts_base_seconds;   /* ORC epoch in the writer timezone (array_decoder/timestamp.rs:133-147); 0 = 1420070400 */
  uint32_t batch_size;       /* rows per RecordBatch, 0 = 8192 (arrow_reader.rs:37)                */
  uint32_t n_streams;
  const orcgpu_stream* streams;
  uint32_t n_columns;
  const orcgpu_column* columns;
  const char* writer_timezone; /* StripeFooter.writer_timezone (stripe.rs:167-171) or NULL.  When given it names a zone of the
                              * system's tz database ($TZDIR, /usr/share/zoneinfo; ORCGPU_UNSUPPORTED if it is not there):
                              * ts_base_seconds is then taken from it and TIMESTAMP columns are re-labelled from that zone
                              * to UTC on the device (array_decoder/timestamp.rs:236-291; values chrono cannot hold become
                              * nulls, as there).  TIMESTAMP_INSTANT columns ignore it. */
} orcgpu_stripe_desc;

/* ---- context ---------------------------------------------------------------------------------- */
/* Returns NULL on failure (no HIP device: the library never falls back to a CPU path). */
orcgpu_ctx* orcgpu_open(int device, const orcgpu_opts* opts);
void orcgpu_close(orcgpu_ctx* ctx);
const char* orcgpu_last_error(const orcgpu_ctx* ctx);
const char* orcgpu_version(void);
/* The binary interface a caller was built against: bumped whenever a struct of this header changes size or layout, or an entry
 * point changes its meaning.  4: device-resident batches (struct ArrowDeviceArray and the *_device entry points) were added;
 * 3 (round 6): orcgpu_lane_stats gained literals_kernel_ms; 2 (round 5): orcgpu_reader_next_batch
 * ends with ORCGPU_END_OF_FILE (110) instead of 1, orcgpu_stream gained skip_bits.  A binding checks orcgpu_abi_version() ==
 * ORCGPU_ABI_VERSION once, after loading the library. */
#define ORCGPU_ABI_VERSION 4
int orcgpu_abi_version(void);

/* ---- staging: host stream bytes -> HBM --------------------------------------------------------- */
/* Copies every stream of the stripe into one HBM arena (taken from a pool) and scans the 3-byte chunk headers
 * (compression.rs:113-123, :244-267; Zstandard: also the frame / block headers) on the host while the bytes are at hand.
 * From that scan every compressed stream gets its part of the block decompressors' tables (chunk, block and item descriptors,
 * its blocks ordered by sequence count, the workspace it needs), relative to the stream: a decode call copies and rebases them.
 * The copy is a pipeline: 16 MiB pieces go through two pinned buffers, filled by a few host threads while the previous
 * piece is on its way (hipMemcpyAsync on a copy stream).  The call does NOT wait for the last piece: decodes wait for
 * it on the device, so staging stripe k + 1 overlaps decoding stripe k (the analogue of the reference's
 * Stripe::new reading ahead, stripe.rs:127-182 / async_arrow_reader.rs:165-280).  The caller's buffers may be
 * reused as soon as the call returns.  The returned handle keeps its own copy of the descriptor. */
int orcgpu_stage_stripe(orcgpu_ctx* ctx, const orcgpu_stripe_desc* desc, orcgpu_staged** out);
void orcgpu_staged_free(orcgpu_staged* s);
uint64_t orcgpu_staged_bytes(const orcgpu_staged* s); /* sum of Stream.length staged in HBM */

/* ---- decode: staged stripes -> Arrow buffers in HBM -------------------------------------------- */
/* Decodes n staged stripes with shared kernel launches.  Device work only; ends with ONE small
 * device-to-host copy (error words, null counts, string byte totals).  results[i] is allocated
 * unless it is passed non-NULL from an earlier decode of a same-shaped stripe (buffer reuse). */
int orcgpu_decode_staged(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results);
/* Convenience: stage + decode one stripe. */
int orcgpu_stripe_decode(orcgpu_ctx* ctx, const orcgpu_stripe_desc* desc, orcgpu_result** out);
void orcgpu_result_free(orcgpu_result* r);

/* ---- result inspection ------------------------------------------------------------------------- */
/* Decode status of the stripe: ORCGPU_OK, or the error of the FIRST failing batch; *batch gets the
 * index of that batch (batches before it are valid, as with the reference's iterator, which
 * yields Ok batches until the failing one: arrow_reader.rs:333-346). */
int orcgpu_result_status(const orcgpu_result* r, uint32_t* batch, uint32_t* column);
uint64_t orcgpu_result_rows(const orcgpu_result* r);
uint32_t orcgpu_result_batches(const orcgpu_result* r);
uint64_t orcgpu_result_arrow_bytes(const orcgpu_result* r); /* value + offset + validity bytes emitted */

/* Raw view of one column of one batch.  Pointers are DEVICE pointers unless copied with
 * orcgpu_result_copy_batch; layouts follow the Arrow columnar format:
 *   values    fixed width data / Boolean bitmap (LSB first) / string bytes of this batch
 *   offsets   length+1 int32, first = 0 (restart per batch, array_decoder/string.rs:139-140)
 *   validity  LSB-first bitmap, NULL when null_count == 0 (array_decoder/mod.rs:247-251) */
typedef struct {
  uint64_t length;
  uint64_t null_count;
  const void* validity;
  const void* values;
  uint64_t values_bytes;
  const int32_t* offsets;
} orcgpu_batch_view;
int orcgpu_result_batch_view(const orcgpu_result* r, uint32_t batch, uint32_t column, orcgpu_batch_view* out);
/* Copies one column-batch to host memory supplied by the caller (sizes from the view). */
int orcgpu_result_copy_batch(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t batch, uint32_t column, void* values,
                             int32_t* offsets, void* validity);

/* ---- dictionary output (ORCGPU_ARROW_DICTIONARY_UTF8) -------------------------------------------------------------------------
 * A column decoded to that target is, batch for batch, an Int32 column: orcgpu_batch_view.values are the keys (values_bytes =
 * 4 * length, offsets = NULL), validity and null count as on the Utf8 path, a null row's key 0.  orcgpu_result_select, the row-group
 * entry points of orcgpu_stream and orcgpu_result_filter treat the keys as an Int32 column's values and leave the dictionary alone
 * (a filter predicate that COMPARES such a column is ORCGPU_UNSUPPORTED, the message naming it; IS [NOT] NULL works).
 * The stripe has ONE dictionary, shared by all its batches, in Arrow Utf8 layout:
 *   DICTIONARY / DICTIONARY_V2 stripe   entry k is the file's entry k (the LENGTH stream's prefix sums over DICTIONARY_DATA,
 *       dictionary_size entries, file order); the keys are the DATA stream's ids.  An id >= dictionary_size or >= 2^31 is
 *       ORCGPU_ARROW at its row: the status names the first failing batch, the batches before it are valid -- what the Utf8 target
 *       reports for the same stripe.  A dictionary that fails to decode, or holds an entry that is not UTF-8 (checked once per entry),
 *       fails the column as on the Utf8 path.
 *   DIRECT / DIRECT_V2 stripe           the identity dictionary: entry k is the k-th non-null value of the stripe (LENGTH prefix sums
 *       over DATA, no slots for nulls), a valid row's key its rank among the valid rows.  A column so has one Arrow type whatever
 *       each stripe's writer chose.  Values that end beyond 2^31 - 1 dictionary bytes: ORCGPU_ARROW at their row.
 * orcgpu_result_export_batch[_device] export the column as format "i" with ArrowSchema.dictionary "u" and ArrowArray.dictionary
 * the stripe's entries; every batch of the stripe refers to the same buffers -- on the host path they come back once, with the
 * result's arena -- and they go when the last batch referring to them is released.  orcgpu_result_arrow_bytes counts them once. */
typedef struct {
  uint64_t length;         /* entries */
  const int32_t* offsets;  /* DEVICE: length + 1, first 0 (NULL: the stripe has no rows, nothing was decoded) */
  const void* values;      /* DEVICE: the entries' bytes */
  uint64_t values_bytes;
} orcgpu_dictionary_view;
/* ORCGPU_INVALID_ARGUMENT for a column that was not decoded to ORCGPU_ARROW_DICTIONARY_UTF8. */
int orcgpu_result_dictionary_view(const orcgpu_result* r, uint32_t column, orcgpu_dictionary_view* out);
/* Copies the dictionary to host memory supplied by the caller (sizes from the view; either pointer may be NULL). */
int orcgpu_result_copy_dictionary(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t column, int32_t* offsets, void* values);

/* ---- row selection --------------------------------------------------------------------------------------- */
/* One run of a RowSelection (src/row_selection.rs:32-52): row_count rows skipped or selected. */
typedef struct {
  uint64_t row_count;
  int32_t skip;  /* nonzero: skip, zero: select */
} orcgpu_row_selector;
/* Applies the stripe's part of a RowSelection to a decoded stripe -- the `row_selection` argument of
 * NaiveStripeDecoder::new_with_selection (src/array_decoder/mod.rs:570-594).  Afterwards the result's batches are the
 * RecordBatches next_with_row_selection yields (mod.rs:302-365): one per select step of at most batch_size rows, in
 * order; orcgpu_result_batches / _batch_view / _copy_batch / _export_batch speak in those batches.  The stripe was
 * decoded whole (the reference's skip_values decodes and discards too, rle_v2/mod.rs:148-175); values and string bytes
 * of a selected batch are used in place, its validity bitmap, Boolean bits and offsets are rebuilt on the device.
 * Selectors are normalised like `From<Vec<RowSelector>>` (row_selection.rs:466-482). */
int orcgpu_result_select(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_row_selector* selectors, uint32_t n);
/* Host only: one stream's share of a RowIndexEntry's positions (row_index.rs:42-50, :204-226; the reference keeps the list
 * and never seeks with it).  `positions` is the entry of ONE row group of ONE column as the ROW_INDEX stream holds it;
 * the streams of the column take their numbers from it in the order PRESENT, DATA, then LENGTH or SECONDARY:
 * a compressed file gives every stream {offset of a chunk header in the stream, bytes into the decompressed chunk}, an
 * uncompressed one {byte offset}; run-length streams add {values of the run at that byte already consumed}, bit streams
 * (PRESENT, Boolean DATA) after that {bits of the current byte consumed}; dictionary streams have no positions.
 * Describe the column as it is in the stripe: `has_present` = it has a PRESENT stream, `compressed` = the file has a
 * compression codec.  Returns the numbers for stream `kind`, or ORCGPU_OUT_OF_SPEC when the entry has not exactly the
 * positions such a column needs (writers that drop an all-ones PRESENT stream drop its positions too). */
int orcgpu_index_entry(const orcgpu_column* column, int has_present, int compressed, const uint64_t* positions, uint32_t n_positions,
                       int32_t kind, orcgpu_stream_entry* out);
/* Host only: the UTC offsets (seconds east of Greenwich) the library uses for a writer time zone at n instants (seconds since
 * the UNIX epoch), and the ORC epoch in that zone (2015-01-01T00:00:00 there, timestamp.rs:133-147; orc_epoch may be NULL).
 * ORCGPU_UNSUPPORTED when the tz database does not have the zone. */
int orcgpu_timezone_offsets(const char* name, const int64_t* instants, uint32_t n, int32_t* offsets, int64_t* orc_epoch);
/* Host only: the stepping by itself.  Splits the first stripe_rows rows off the selection (RowSelection::split_off,
 * row_selection.rs:278-314), runs next_with_row_selection over them and reports the batches as row ranges of the stripe
 * (starts / lens, at most cap of them; *n_out = how many there are) and what is left of the selection (rest). */
int orcgpu_selection_batches(const orcgpu_row_selector* selectors, uint32_t n, uint64_t stripe_rows, uint32_t batch_size, uint64_t* starts,
                             uint32_t* lens, uint32_t cap, uint32_t* n_out, orcgpu_row_selector* rest, uint32_t rest_cap, uint32_t* n_rest);

/* Brings every Arrow buffer of the result to the host at once: one hipMemcpyAsync per result arena into pinned memory
 * (the counterpart of the reference handing out freshly allocated host buffers, array_decoder/mod.rs:100-120), one
 * synchronisation.  orcgpu_result_export_batch calls it on demand; the exported batches are views into that copy and
 * keep it alive after orcgpu_result_free. */
int orcgpu_result_fetch(orcgpu_ctx* ctx, orcgpu_result* r);
/* The same without the wait: the copies are enqueued on the context's device-to-host stream (behind the work enqueued on the
 * decode stream so far) and the call returns; the next stripe can be staged and decoded meanwhile.  orcgpu_result_fetch /
 * _export_batch wait for them; decoding into the result again, selecting on it or freeing it waits too.  With
 * orcgpu_stage_stripe (which does not wait for its copies either) this is what lets a caller keep three stripes in flight:
 * staging k + 1, decoding k, copying k - 1 back -- the analogue of the reference's async reader fetching the next stripe
 * while the current one is consumed (async_arrow_reader.rs:165-280). */
int orcgpu_result_fetch_async(orcgpu_ctx* ctx, orcgpu_result* r);

/* ---- Arrow C Data Interface export (https://arrow.apache.org/docs/format/CDataInterface.html) ---- */
struct ArrowSchema;
struct ArrowArray;
struct ArrowDeviceArray;
/* The three are incomplete types here: a caller brings its own definitions (Arrow's abi.h, arrow::ffi, a restatement of the
 * specification).  A caller that wants them from this header defines ORCGPU_ARROW_STRUCTS before including it. */
#ifdef ORCGPU_ARROW_STRUCTS
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif
/* The Arrow C Device Data Interface (https://arrow.apache.org/docs/format/CDeviceDataInterface.html): an ArrowArray whose buffer
 * pointers are device memory, the device they live on, and an event to wait for before reading them. */
#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  int32_t device_type;  /* ARROW_DEVICE_* */
  void* sync_event;     /* ROCm: a hipEvent_t*, or NULL when no synchronisation is needed */
  int64_t reserved[3];
};
#endif
#endif /* ORCGPU_ARROW_STRUCTS */
/* Exports batch `batch` as a struct array (one child per projected column) into HOST memory owned
 * by the release callbacks; a Rust caller imports it with arrow::ffi::from_ffi, Python with
 * pyarrow.RecordBatch._import_from_c.  Field names are "c<column_id>"; the caller renames. */
int orcgpu_result_export_batch(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t batch, struct ArrowArray* out_array,
                               struct ArrowSchema* out_schema);

/* ---- file reader: host-side mirror of ArrowReaderBuilder / ArrowReader ---------------------------------- */
/* The container layer around the hot path, restated in C++ inside liborcgpu.so because it produces
 * the kernel inputs: ChunkReader (src/reader/mod.rs:27-76), read_metadata (src/reader/metadata.rs:
 * 180-247), Stripe::new (src/stripe.rs:127-182), ProjectionMask::named_roots (src/projection.rs:52-69),
 * ArrowReaderBuilder::{try_new, with_batch_size, with_projection, with_file_byte_range,
 * with_timestamp_precision, build} (src/arrow_reader.rs:70-231) and ArrowReader::{next,
 * total_row_count} (:243-346).  Setters must be called before the first next_batch ("build"). */
typedef struct orcgpu_reader orcgpu_reader;
int orcgpu_reader_open_file(orcgpu_ctx* ctx, const char* path, orcgpu_reader** out);                 /* try_new(File)  */
int orcgpu_reader_open_bytes(orcgpu_ctx* ctx, const uint8_t* data, uint64_t len, orcgpu_reader** out); /* try_new(Bytes) */
void orcgpu_reader_close(orcgpu_reader* r);
int orcgpu_reader_set_batch_size(orcgpu_reader* r, uint32_t batch_size);                             /* with_batch_size */
int orcgpu_reader_set_projection(orcgpu_reader* r, const char* const* root_names, uint32_t n);       /* named_roots     */
int orcgpu_reader_set_projection_roots(orcgpu_reader* r, const uint32_t* root_indices, uint32_t n);  /* ProjectionMask::roots (projection.rs:37): indices of root columns */
/* with_schema (arrow_reader.rs:80): the Arrow schema to decode into, as an Arrow C Data Interface struct ("+s") whose
 * children are matched with the projected root columns by position (NaiveStripeDecoder::new zips columns and fields,
 * array_decoder/mod.rs:577-582).  Field names become the batches' column names; a type pair the reference has no decoder
 * for makes the first orcgpu_reader_next_batch return ORCGPU_MISMATCHED_SCHEMA.  The schema is read, not consumed. */
int orcgpu_reader_set_schema(orcgpu_reader* r, const struct ArrowSchema* schema);
int orcgpu_reader_set_byte_range(orcgpu_reader* r, uint64_t start, uint64_t end);                    /* with_file_byte_range */
/* Dictionary output (opt-in; the reference has no counterpart): the named columns -- projected root columns of ORC kind STRING /
 * VARCHAR / CHAR -- come as Dictionary(Int32, Utf8) instead of Utf8: ORCGPU_ARROW_DICTIONARY_UTF8 in every stripe, whatever its
 * encoding there.  Before the first batch; n = 0 restores the default.  A name the file's root columns do not have, a name given
 * twice, a column of another kind: ORCGPU_INVALID_ARGUMENT, the message naming it (a name outside the projection is met at the
 * first batch, the same way).  With orcgpu_reader_set_schema the field of such a column must be Utf8.  Everything else --
 * projection, shards, byte ranges, row selection, pruning, read-ahead, compression -- works as before; a row filter may not
 * compare such a column (ORCGPU_UNSUPPORTED). */
int orcgpu_reader_set_dictionary_columns(orcgpu_reader* r, const char* const* names, uint32_t n);
/* `world` processes, one per GPU, read ONE file together; this reader is number `rank` of them.  The units of the
 * path are independent (stripe.rs:154-165: a stripe's columns are decoded one by one), so no data is exchanged -- each reader
 * reads, stages and decodes only what is its own; what the ranks do with their batches (an all-gather of row counts,
 * concatenation by column or by stripe) is the caller's.  The reference's own split hook is a byte range per reader
 * (arrow_reader.rs:86-89, :358-372).
 *   ORCGPU_SHARD_STRIPES  stripe k (of those the byte range leaves) belongs to rank k % world: whole stripes, every projected
 *                         column.  A row selection is stepped through every stripe, read or not, so the ranks' batches put
 *                         together in stripe order are the batches of a single reader.
 *   ORCGPU_SHARD_COLUMNS  the projected root columns are dealt out by their estimated Arrow bytes per row (orcgpu_shard_columns:
 *                         largest first, to the least loaded rank): every rank reads every stripe, its own columns only; its
 *                         batches have the same rows as a single reader's, the ranks' columns put side by side are its columns.
 * world = 1 (the default) reads everything. */
enum { ORCGPU_SHARD_STRIPES = 0, ORCGPU_SHARD_COLUMNS = 1 };
int orcgpu_reader_set_shard(orcgpu_reader* r, uint32_t rank, uint32_t world, int mode);
/* The column deal alone (host only, no GPU): rank_of[i] for n columns of the given weights.  Longest-processing-time rule:
 * columns in order of falling weight (ties: the earlier column first), each to the rank with the least weight so far (ties:
 * the lower rank).  What orcgpu_reader_set_shard(.., ORCGPU_SHARD_COLUMNS) uses, with orcgpu_reader_column_weight's weights. */
int orcgpu_shard_columns(const double* weights, uint32_t n, uint32_t world, uint32_t* rank_of);
/* Estimated Arrow bytes per row of root column `root` of the file (its index among the root columns): fixed widths, 16 for
 * Decimal128, 4 + 16 for strings and binaries, the sum of its fields for a Struct, offsets + two elements for Lists and Maps. */
double orcgpu_reader_column_weight(const orcgpu_reader* r, uint32_t root);
int orcgpu_reader_set_timestamp_precision(orcgpu_reader* r, int arrow_target);                       /* ORCGPU_ARROW_TIMESTAMP_* */
/* with_row_selection (arrow_reader.rs:113): a selection over the rows of the FILE; every stripe takes its share with
 * RowSelection::split_off, and once no rows are left in the selection later stripes are read whole (arrow_reader.rs:296-308). */
int orcgpu_reader_set_row_selection(orcgpu_reader* r, const orcgpu_row_selector* selectors, uint32_t n);
/* Row groups under a row selection (default: on).  The reference decodes a stripe from its first row and discards what a
 * selection skips (skip_values, rle_v2/mod.rs:148-175).  This reader reads the stripe's ROW_INDEX streams (row_index.rs:204-226)
 * and reads, stages and decodes only the row groups (rowIndexStride rows, stripe.rs:300) that hold selected rows -- every
 * stream from the entry point its index names, consecutive row groups together; a stripe without selected rows is not read
 * at all.  The batches are the ones the whole decode yields.  Stripes without usable indexes (no ROW_INDEX streams, an entry
 * that does not fit its column, bit streams entered in mid-byte, List / Map columns) are decoded whole.  What differs, on
 * damaged files only: an error inside row groups that are not read is not met.  `on` = 0 turns it off. */
int orcgpu_reader_set_row_group_pruning(orcgpu_reader* r, int on);
/* How many row groups the reader has read and how many the stripes it went through hold (whole stripes count all of theirs). */
int orcgpu_reader_row_groups(const orcgpu_reader* r, uint64_t* read, uint64_t* total);
/* ---- predicate pushdown onto row groups (src/predicate.rs, src/row_group_filter.rs, arrow_reader.rs:173, :258-308) ---- */
/* A Predicate as a list of nodes in pre-order: a node, then its children one after the other (AND / OR: n_children of them,
 * NOT: one; comparisons and null tests: none). */
enum { ORCGPU_PRED_EQ = 0, ORCGPU_PRED_NE = 1, ORCGPU_PRED_LT = 2, ORCGPU_PRED_LE = 3, ORCGPU_PRED_GT = 4, ORCGPU_PRED_GE = 5, /* ComparisonOp */
       ORCGPU_PRED_IS_NULL = 6, ORCGPU_PRED_IS_NOT_NULL = 7, ORCGPU_PRED_AND = 8, ORCGPU_PRED_OR = 9, ORCGPU_PRED_NOT = 10,
       /* (11 .. 15: unknown ops) */
       ORCGPU_PRED_LIKE = 16 /* SQL LIKE, this library's own: a leaf with column, value_type = ORCGPU_PV_UTF8, s / s_len = the pattern,
                                i = the escape byte (0: none, else 1 .. 127), value_is_null = the NULL pattern; see orcgpu_result_filter */,
       ORCGPU_PRED_IN = 17 /* SQL IN, this library's own: a leaf with column; n_children counts the ORCGPU_PRED_LITERAL nodes that
                              follow it in pre-order, its list.  There is no NOT IN: put ORCGPU_PRED_NOT above the leaf */,
       ORCGPU_PRED_LITERAL = 18 /* one value of an IN list: column = NULL, n_children = 0; value_type, value_is_null, i, f, s, s_len as
                                   in a comparison node.  Anywhere but under an ORCGPU_PRED_IN it is ORCGPU_INVALID_ARGUMENT */,
       ORCGPU_PRED_CMP_EXPR = 19 /* lhs OP rhs over two arithmetic expressions, this library's own: a leaf with column = NULL,
                                    i = ORCGPU_PRED_EQ .. _GE and n_children = 2; the two expression subtrees follow it in pre-order,
                                    the left side first.  See orcgpu_result_filter */,
       /* the nodes of such a subtree: the language of orcgpu_agg_expr_node, with every field where that struct has it */
       ORCGPU_PRED_EXPR_COLUMN = 20 /* `column`: a projected root column; no children */,
       ORCGPU_PRED_EXPR_LITERAL = 21 /* value_type ORCGPU_PV_INT64: i; _FLOAT64: f; _DECIMAL128: s / s_len / i; no children */,
       ORCGPU_PRED_EXPR_ADD = 22, ORCGPU_PRED_EXPR_SUB = 23, ORCGPU_PRED_EXPR_MUL = 24 /* exactly two children */,
       ORCGPU_PRED_EXPR_NEG = 25 /* exactly one child */,
       ORCGPU_PRED_IN_SET = 26 /* x IN SET s, this library's own: a leaf with column and i = orcgpu_key_set_id of a sealed key set of
                                  the same context; no children.  There is no NOT IN SET: put ORCGPU_PRED_NOT above the leaf.  See
                                  "key sets" below */,
       ORCGPU_PRED_EXPR_DATE_PART = 36 /* an expression node like 20 .. 25 (ORCGPU_AGG_EXPR_DATE_PART + 20): exactly one child,
                                          i = ORCGPU_DATE_PART_*.  A leaf that holds one keeps every row group when pruning */,
       ORCGPU_PRED_EXPR_DIV = 37, ORCGPU_PRED_EXPR_FLOOR_DIV = 38, ORCGPU_PRED_EXPR_MOD = 39
                                       /* a / b, a // b, a % b: expression nodes like 20 .. 25 (ORCGPU_AGG_EXPR_DIV .. _MOD + 20), exactly
                                          two children; DIV: i = the result scale 0 .. 38, or -1 (the expression aggregates' DIVISION).
                                          A leaf that holds one keeps every row group when pruning */,
       /* (40: an unknown op) */
       ORCGPU_PRED_EXPR_IF = 41, ORCGPU_PRED_EXPR_COALESCE = 42, ORCGPU_PRED_EXPR_ABS = 43, ORCGPU_PRED_EXPR_NULL = 44,
       ORCGPU_PRED_EXPR_CMP = 45, ORCGPU_PRED_EXPR_IS_NULL = 46, ORCGPU_PRED_EXPR_AND = 47, ORCGPU_PRED_EXPR_OR = 48,
       ORCGPU_PRED_EXPR_NOT = 49      /* the conditional nodes of an expression (ORCGPU_AGG_EXPR_IF .. _NOT + 20; the expression
                                          aggregates' CONDITIONALS): 3, 2, 1, 0, 2, 1, 2, 2, 1 children; CMP: i = ORCGPU_PRED_EQ .. _GE.
                                          A leaf that holds one keeps every row group when pruning */,
       ORCGPU_PRED_EXPR_CAST = 50, ORCGPU_PRED_EXPR_ROUND = 51, ORCGPU_PRED_EXPR_FLOOR = 52, ORCGPU_PRED_EXPR_CEIL = 53,
       ORCGPU_PRED_EXPR_TRUNC = 54    /* the conversion nodes of an expression (ORCGPU_AGG_EXPR_CAST .. _TRUNC + 20; the expression
                                          aggregates' CONVERSIONS): exactly one child each; CAST: value_type = the target, i = the scale of
                                          a DECIMAL128 target; ROUND: i = the digits.  A leaf that holds one keeps every row group when
                                          pruning */ };
/* What one IN list may hold: literal nodes (before duplicates are dropped), and bytes of Utf8 literals in all. */
#define ORCGPU_IN_MAX_VALUES 65536
#define ORCGPU_IN_MAX_BYTES (4u << 20)
/* What a LIKE pattern may hold after unescaping: bytes (wildcards included) and non-empty parts between its `%` signs.  The
 * compiled pattern then fits the matcher kernel's LDS. */
#define ORCGPU_LIKE_MAX_BYTES 1024
#define ORCGPU_LIKE_MAX_PARTS 64
/* PredicateValue (predicate.rs:29-47), and two kinds the reference does not have:
 *   ORCGPU_PV_DECIMAL128    s -> the 16 bytes of the unscaled value, little-endian two's complement, s_len = 16; i = the literal's
 *                           scale, 0 .. 38; |unscaled| < 10^38.  Anything else is ORCGPU_INVALID_ARGUMENT (the message names the column).
 *   ORCGPU_PV_TIMESTAMP_NS  i = nanoseconds since 1970-01-01T00:00:00 in the sense of the exported Arrow value: naive wall clock
 *                           for a TIMESTAMP column, UTC for TIMESTAMP_INSTANT.  The literal's range is int64's: 1677-09-21 to 2262-04-11. */
enum { ORCGPU_PV_BOOLEAN = 0, ORCGPU_PV_INT8 = 1, ORCGPU_PV_INT16 = 2, ORCGPU_PV_INT32 = 3, ORCGPU_PV_INT64 = 4, ORCGPU_PV_FLOAT32 = 5,
       ORCGPU_PV_FLOAT64 = 6, ORCGPU_PV_UTF8 = 7, ORCGPU_PV_DECIMAL128 = 8, ORCGPU_PV_TIMESTAMP_NS = 9 };
typedef struct {
  int32_t op;            /* ORCGPU_PRED_*                                                                 */
  uint32_t n_children;   /* AND / OR; IN: the literal nodes of its list                                    */
  const char* column;    /* comparisons and null tests: the name of a projected root column               */
  int32_t value_type;    /* comparisons: ORCGPU_PV_*                                                       */
  int32_t value_is_null; /* ... Some / None                                                                */
  int64_t i;             /* Boolean (0 / 1) and the integer kinds; Decimal128: the scale; TimestampNs      */
  double f;              /* Float32 / Float64                                                              */
  const char* s;         /* Utf8: bytes, not necessarily terminated; Decimal128: the 16 bytes              */
  uint64_t s_len;
} orcgpu_predicate_node;
/* What the reader knows about one column of one stripe: the plain (decompressed) bytes of its ROW_INDEX stream, a
 * proto RowIndex, and of its BLOOM_FILTER (else BLOOM_FILTER_UTF8) stream, a proto BloomFilterIndex (NULL, 0: none). */
typedef struct {
  const char* name;
  const uint8_t* row_index;
  uint64_t row_index_len;
  const uint8_t* bloom_index;
  uint64_t bloom_index_len;
} orcgpu_column_index;
/* Host only: evaluate_predicate (row_group_filter.rs:50-165) -- which row groups of a stripe might hold rows that satisfy the
 * predicate, judged by the row groups' statistics (min / max, null counts: :167-330, :470-620) and, for equality, their Bloom
 * filters (:332-371, bloom_filter.rs).  keep[g] = 1: row group g must be read; *n_groups = ceil(stripe_rows / rows_per_group)
 * (keep must have room for that many).  Anything but ORCGPU_OK means the reference's evaluation fails (a column that is not
 * there or has no index, a value of the wrong type, a row group without typed statistics): its reader then reads every row. */
int orcgpu_predicate_row_groups(const orcgpu_predicate_node* nodes, uint32_t n_nodes, const orcgpu_column_index* columns, uint32_t n_columns,
                                uint64_t stripe_rows, uint64_t rows_per_group, uint8_t* keep, uint32_t* n_groups);
/* with_predicate (arrow_reader.rs:173): per stripe the predicate is evaluated against the stripe's row indexes, the row groups
 * it keeps become a RowSelection (RowSelection::from_row_group_filter, row_selection.rs:348-392) and the stripe is decoded under
 * it -- here: only those row groups are read (orcgpu_reader_set_row_group_pruning).  A stripe whose evaluation fails is read
 * whole.  The nodes (and their strings) are copied.  With a row selection as well, a row is read when both select it (the
 * reference's own combination, arrow_reader.rs:296-308, panics unless the row selection selects every row of the stripe). */
int orcgpu_reader_set_predicate(orcgpu_reader* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes);
/* ---- row filter: a predicate evaluated per ROW on the device, before the copy back ------------------------------------------
 * with_predicate (above) prunes whole row groups, as the reference does; every row of a kept row group is still decoded, copied
 * back and exported.  A row filter evaluates the predicate on every decoded row on the device and compacts the rows it keeps
 * (device/filter_kernels.hip), so that only those cross the link.  The reference has no row-level evaluation; the semantics are
 * fixed here:
 *   - SQL three-valued logic; a row is kept only when the root is TRUE.
 *   - A comparison is UNKNOWN when the row is null or the literal is None (value_is_null).  IS NULL / IS NOT NULL are never
 *     UNKNOWN.  AND / OR are Kleene (an AND of no children is TRUE, an OR of none FALSE); NOT UNKNOWN = UNKNOWN.
 *   - Byte / Short / Int / Long columns take any of the Int8 .. Int64 literals and compare as int64.  Date takes Int32 / Int64
 *     literals, as days.  Float / Double take Float32 / Float64 literals and compare as double (a Float32 literal is rounded
 *     through float first); IEEE rules: with a NaN on either side EQ / LT / LE / GT / GE are FALSE and NE is TRUE, -0.0 == 0.0.
 *     Boolean takes Boolean, false < true.  String / Varchar / Char / Binary take Utf8 and compare the decoded value as exported
 *     by unsigned byte, the shorter one being the smaller on a common prefix.  Any other pair: ORCGPU_MISMATCHED_SCHEMA.
 *   - Decimal takes Decimal128 and compares in exact rational order, unscaled_c * 10^-scale_c against unscaled_l * 10^-scale_l,
 *     whatever the two scales.  Timestamp and Timestamp-instant take TimestampNs and compare as instants: the exported int64 in
 *     its unit (s, ms, us, ns) against the literal's nanoseconds, exactly -- a literal between two values of the unit equals no
 *     row.  The host brings the literal to the column's scale / unit (floor, with the operator adjusted where it does not
 *     divide; clamped where it leaves int128), the device compares integers and rescales no row.  Any other literal kind on
 *     these columns, and a Timestamp column decoded to Decimal128(38, 9), is ORCGPU_UNSUPPORTED (the message names the column);
 *     a Decimal128 or TimestampNs literal on any other column is ORCGPU_MISMATCHED_SCHEMA.
 *   - ORCGPU_PRED_LIKE on a String / Varchar / Char column with a Utf8 pattern.  The pattern is matched against the WHOLE exported
 *     value of the row (a Char value with its padding).  `%` matches any run of bytes, none included; `_` matches exactly one
 *     UTF-8 code point of the value (a lead byte with the continuation bytes 10xxxxxx behind it; a newline is a character like
 *     any other); the escape byte (node.i; 0: none) makes the pattern byte behind it a literal, whatever that byte is; every other
 *     pattern byte matches itself, as an unsigned byte -- the pattern need not be valid UTF-8.  A null row and the NULL pattern
 *     are UNKNOWN; there is no NOT LIKE: put ORCGPU_PRED_NOT above the leaf (a null row is dropped either way).  A Binary
 *     column, any other column kind and any other value_type: ORCGPU_MISMATCHED_SCHEMA.  A pattern that ends in its escape byte
 *     and an escape outside 0 .. 127: ORCGPU_INVALID_ARGUMENT.  A pattern of more than ORCGPU_LIKE_MAX_BYTES bytes after
 *     unescaping or more than ORCGPU_LIKE_MAX_PARTS non-empty parts between its `%`: ORCGPU_UNSUPPORTED (the compiled pattern is
 *     held in the matcher kernel's LDS).  A column read as a dictionary column: ORCGPU_UNSUPPORTED, as for a comparison.  Each
 *     message names the column.  The pattern is matched by a kernel of its own (filter_like_kernel) in front of the evaluation,
 *     on the same stream: no further host wait.
 *   - ORCGPU_PRED_IN: x IN (v1, ..., vk) is exactly OR(x = v1, ..., x = vk) under the rules above, and everything follows from that.
 *     A null row is UNKNOWN.  The empty list is FALSE for every row, null rows included (an OR of no children).  A NULL literal in
 *     the list (value_is_null) turns every non-match into UNKNOWN: NOT IN over a list with a NULL keeps nothing, a list of nothing
 *     but NULLs is UNKNOWN everywhere.  Duplicates are harmless.  Every literal is checked against the column as the literal of an
 *     EQ is, with the same statuses and messages; the literal kinds may be mixed within what the column takes.  Float columns
 *     compare as double: a NaN literal equals no row, -0.0 and 0.0 are one key, a Float32 literal is rounded through float first.
 *     Decimal128 and TimestampNs literals are brought to the column's scale / unit as for EQ; one that does not land on a value of
 *     the scale / unit equals no row (FALSE on valid rows, no error).  A column read as a dictionary column, a nested column among
 *     the columns and a Timestamp column decoded to Decimal128(38, 9): ORCGPU_UNSUPPORTED, as for a comparison.  More than
 *     ORCGPU_IN_MAX_VALUES literal nodes or more than ORCGPU_IN_MAX_BYTES bytes of Utf8 literals in one list: ORCGPU_UNSUPPORTED
 *     (the message names the column).  A literal node anywhere but under an IN, an IN child that is not a literal node, a literal
 *     node with children and a node list that ends inside the list: ORCGPU_INVALID_ARGUMENT.  The list counts toward
 *     ORCGPU_FILTER_MAX_DEPTH as the leaf alone.  One distinct key (and no NULL) is compiled to the comparison EQ.  Otherwise the
 *     keys go into a hash set (open addressing, linear probing) that a kernel of its own (filter_in_kernel) probes per row in front
 *     of the evaluation, on the same stream: from LDS when the table is at most 32 KiB, else where it lies in global memory; no
 *     further host wait.  The cost per row does not grow with the list.
 *   - ORCGPU_PRED_CMP_EXPR: lhs OP rhs.  Each side is an arithmetic expression in the language of the expression aggregates
 *     (orcgpu_result_aggregate_exprs: columns, literals, + - *, unary -), OP one of EQ .. GE, evaluated exactly, per row.
 *     CLASSES, decided over BOTH sides together: INT (Byte .. Long columns and INT64 literals; a Date column takes part as int64
 *     days -- in this leaf only, SUM over a Date column is refused as before), DEC (at least one Decimal column or DECIMAL128
 *     literal on either side; integers beside them are Decimals of scale 0; the scale rule is that of the expression aggregates,
 *     a node past scale 38 is ORCGPU_UNSUPPORTED) and FLOAT (Float / Double columns and FLOAT64 literals, every operation one IEEE
 *     double operation).  Float and exact operands do not mix: ORCGPU_MISMATCHED_SCHEMA, naming the column.  A Boolean, String /
 *     Varchar / Char / Binary or Timestamp column, a nested one and one read as a dictionary column: ORCGPU_UNSUPPORTED, naming it.
 *     THE COMPARISON: INT compares as int128.  FLOAT compares as a Float leaf does (a NaN on either side makes all but NE false,
 *     -0.0 == 0.0).  DEC compares in exact rational order: the side of the smaller scale is multiplied by 10^d, d the difference
 *     of the two sides' scales; where that product leaves 128 bits the order is still exact -- a positive side that overflows is
 *     greater than any int128, a negative one smaller.  No row is UNKNOWN because of this final rescale.
 *     UNKNOWN on a row where a column of either side is NULL, and on a row where an operation INSIDE a side leaves 128 bits: the
 *     value does not exist, as for a NULL; nothing wraps.  The row filter counts the latter (row, leaf) evaluations:
 *     orcgpu_reader_filter_overflow_rows (0 unless something overflowed; the count travels in the filter's one host wait).  As an
 *     aggregate's condition and as the filter of a top-k the rule holds and the count is not surfaced.
 *     SIMPLE FORMS: a side of literals alone is folded.  A bare column against a side that folds to a literal the column's own
 *     comparison takes (an integer or Date column and a literal within int64; a Float / Double column; a Decimal column and a
 *     literal of |value| < 10^38) compiles to that comparison, the operator mirrored when the column stands on the right -- and
 *     orcgpu_predicate_row_groups prunes it as that comparison when the literal side is ONE literal node; two literal sides
 *     compile to TRUE / FALSE.  Every other expression leaf is a sound "might match" for row-group pruning: it keeps every group
 *     and never fails the evaluation; a leaf that holds a date part (ORCGPU_PRED_EXPR_DATE_PART: the expression aggregates' DATE
 *     PARTS, with the overflow of an operand outside int32 UNKNOWN and counted like any other) is always such a leaf, and so is one
 *     that holds a division (ORCGPU_PRED_EXPR_DIV / _FLOOR_DIV / _MOD: the expression aggregates' DIVISION; a zero divisor is an
 *     overflow, so the row is UNKNOWN and counted).  LIMITS: each side at most ORCGPU_AGG_EXPR_MAX_NODES nodes and ORCGPU_AGG_EXPR_MAX_DEPTH
 *     operand slots (the balanced 16-leaf tree is refused); the leaf counts toward ORCGPU_FILTER_MAX_DEPTH as a leaf alone.  An
 *     expression node anywhere but under an ORCGPU_PRED_CMP_EXPR, a wrong child count, a node list that ends inside a subtree,
 *     a comparison op outside 0 .. 5: ORCGPU_INVALID_ARGUMENT.  Both sides are evaluated by a kernel of its own
 *     (filter_expr_kernel) in front of the evaluation, on the same stream, into two planes (TRUE, FALSE): no further host wait.
 *   - A Struct, List, Map or Union column among the columns: ORCGPU_UNSUPPORTED.
 *   - A leaf naming a column that is not there, a leaf without a name, an unknown op, a node list that ends inside a node's
 *     children or goes on behind the root, and a predicate nested deeper than ORCGPU_FILTER_MAX_DEPTH levels (a leaf alone is
 *     one level): ORCGPU_INVALID_ARGUMENT.
 * The nodes are those of orcgpu_reader_set_predicate (pre-order). */
#define ORCGPU_FILTER_MAX_DEPTH 64
/* The analogue of orcgpu_result_select for a filter: applies to a decoded result whose batches are uniform or already selected.
 * Afterwards the result's batches are the kept rows of those batches, in order, packed into batches of at most batch_size rows
 * (only the last may be shorter; no kept row: 0 batches); orcgpu_result_rows / _batches / _batch_view / _copy_batch / _fetch /
 * _fetch_async / _export_batch speak of them, and a copy back moves the kept rows only.  column_names[i] names the result's
 * column i for the leaves (n_columns = the result's columns).  *rows_kept (may be NULL) gets the kept row count.  A result whose
 * orcgpu_result_status is not OK is left as it is, and that status is returned.  A batch of kept rows whose string bytes exceed
 * INT32_MAX fails like a decoded one (ORCGPU_OFFSET_OVERFLOW in orcgpu_result_status).  One host wait per call. */
int orcgpu_result_filter(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                         const char* const* column_names, uint32_t n_columns, uint64_t* rows_kept);
/* A builder setter (before the first next_batch; the nodes and their strings are copied): every stripe's result is filtered
 * after decoding -- and after the row selection if there is one: a row is returned when the selection selects it and the filter
 * keeps it --, before its copy back is started, with and without read-ahead.  The leaves name projected root columns.  Stripes
 * are not merged: a stripe's kept rows come in batches of batch_size rows, its last one shorter; a stripe without kept rows
 * yields no batch.  By itself the filter prunes no row groups: set the same predicate with orcgpu_reader_set_predicate for that
 * (under a row filter the row groups read of a stripe are ONE run, from the first to the last group wanted, so that a stripe's
 * kept rows stay together).  Errors are loud: what orcgpu_result_filter refuses, the first orcgpu_reader_next_batch returns,
 * and the iterator ends. */
int orcgpu_reader_set_row_filter(orcgpu_reader* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes);
/* Rows the row filter has seen (decoded rows, those of the row selection when there is one) and kept so far. */
int orcgpu_reader_filter_rows(const orcgpu_reader* r, uint64_t* rows_seen, uint64_t* rows_kept);
/* (row, expression leaf) evaluations of the row filter so far in which an operation inside a side of an ORCGPU_PRED_CMP_EXPR left
 * 128 bits: the leaf was UNKNOWN there.  0 unless something overflowed.  Aggregates' conditions and the top-k's filter do not
 * count. */
int orcgpu_reader_filter_overflow_rows(const orcgpu_reader* r, uint64_t* rows);
/* ---- aggregates over the kept rows: COUNT, SUM, MIN, MAX and SUM(a * b), reduced on the device ------------------------------
 * A row filter hands the kept rows out; a query like TPC-H Q6 wants one number of them.  An aggregate list is reduced where the
 * decoded rows lie (device/agg_kernels.hip), from the keep mask the filter's evaluation leaves: nothing is scanned, placed,
 * gathered or copied back but one record per aggregate.  The reference has no aggregation; the semantics are fixed here.
 *   - A KEPT row is one the row selection selects (if there is one) and for which the row filter's root is TRUE (if there is
 *     one, under the rules above).  With neither, every row is kept.
 *   - Null values are skipped; SUM_PRODUCT skips a row when either operand is null.  SUM, MIN, MAX and SUM_PRODUCT over no value
 *     are NULL (is_null = 1); the counts are 0.
 *   - COUNT_ROWS (no column): the kept rows.  COUNT: the kept rows whose value is not null; any root column, dictionary columns
 *     included (String and Binary columns take COUNT only).  Both are ORCGPU_AGG_KIND_U64.
 *   - SUM takes Byte .. Long, Float, Double and Decimal.  SUM_PRODUCT takes two Byte .. Long columns, two Float / Double columns
 *     or two Decimal columns (a column with itself is fine).
 *       Integers: SUM is exact as a signed 128-bit integer; SUM_PRODUCT multiplies exactly in 128 bits and accumulates in 192
 *       bits.  ORCGPU_AGG_KIND_I128 in w[0..1]; overflow = 1 when the final value does not fit 128 bits.  The accumulators are wide
 *       enough for every partial sum, so the result does not depend on the order of summation.
 *       Decimal: the unscaled values are accumulated in 192 bits at the column's scale; SUM_PRODUCT at the scale s1 + s2 (more
 *       than 38: ORCGPU_UNSUPPORTED, the message names the columns).  ORCGPU_AGG_KIND_DEC128 in w[0..1] with scale_or_unit = the
 *       scale; overflow = 1 when the final |sum| >= 10^38, and -- SUM_PRODUCT, sticky -- when an operand of a row does not fit a
 *       signed 64-bit word (Decimal(18, s) and narrower always fit).  The value of a result with overflow = 1 is unspecified.
 *       Float / Double: accumulated as double (a Float32 widened first, a product rounded once); NaN and inf - inf give NaN as
 *       IEEE says.  ORCGPU_AGG_KIND_F64 in f.  The sum is DETERMINISTIC: the same result, selection, filter and batch size give the
 *       same bits on every run (a reduction of fixed shape, no floating-point atomics) -- but not the bits of another order.
 *   - MIN, MAX take Byte .. Long, Date (days), Boolean (0 / 1) and Timestamp / Timestamp-instant decoded to an int64 unit:
 *     ORCGPU_AGG_KIND_I64 in w[0], scale_or_unit = a Timestamp's unit (0 s, 1 ms, 2 us, 3 ns), else -1; Decimal: ORCGPU_AGG_KIND_DEC128
 *     at the column's scale; Float / Double: ORCGPU_AGG_KIND_F64, NaN values skipped unless every kept non-null value is NaN, in
 *     which case the result is NaN; -0.0 and 0.0 compare equal, either may come back.
 *   - Any other (op, column kind) pair, and a SUM_PRODUCT of mixed kinds: ORCGPU_MISMATCHED_SCHEMA.  SUM, MIN, MAX or SUM_PRODUCT on
 *     a column read as a dictionary column, or on a Timestamp decoded to Decimal128(38, 9): ORCGPU_UNSUPPORTED.  A nested column in
 *     the result: ORCGPU_UNSUPPORTED.  A column that is not a projected root column, no spec or more than ORCGPU_AGG_MAX of them, an
 *     unknown op: ORCGPU_INVALID_ARGUMENT.  Every message names the column. */
#define ORCGPU_AGG_MAX 64
enum { ORCGPU_AGG_OP_COUNT_ROWS = 0, ORCGPU_AGG_OP_COUNT = 1, ORCGPU_AGG_OP_SUM = 2, ORCGPU_AGG_OP_MIN = 3, ORCGPU_AGG_OP_MAX = 4, ORCGPU_AGG_OP_SUM_PRODUCT = 5 };
enum { ORCGPU_AGG_KIND_U64 = 0, ORCGPU_AGG_KIND_I128 = 1, ORCGPU_AGG_KIND_DEC128 = 2, ORCGPU_AGG_KIND_F64 = 3, ORCGPU_AGG_KIND_I64 = 4 };
typedef struct {
  uint32_t op;          /* ORCGPU_AGG_OP_* */
  const char* column;   /* NULL for COUNT_ROWS */
  const char* column2;  /* SUM_PRODUCT: the second operand */
} orcgpu_agg_spec;
typedef struct {
  uint32_t kind;        /* ORCGPU_AGG_KIND_* */
  uint32_t is_null, overflow;
  int32_t scale_or_unit;
  uint64_t w[3];        /* little-endian words, two's complement: the count, the integer, the unscaled value */
  double f;
} orcgpu_agg_value;
/* Aggregates the rows of a decoded result -- uniform, selected, or the kept rows a row filter left in it -- that the predicate
 * keeps (n_nodes = 0: no filter).  column_names[i] names the result's column i for the leaves and the specs; out gets n_specs
 * values.  The result is read and left as it was: the call may be repeated, and a filter applied afterwards gives what it gives
 * without it.  A result whose status is not OK is refused with that status.  One host wait per call. */
int orcgpu_result_aggregate(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                            const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs, uint32_t n_specs,
                            orcgpu_agg_value* out);
/* A builder setter (before the first call; the specs and their strings are copied): the reader aggregates instead of handing
 * out batches.  orcgpu_reader_aggregate then drains it -- every stripe it would read, under everything the builder set:
 * projection, byte range, shard, timestamp precision, row selection, predicate and pruning, row filter, read-ahead -- and per
 * stripe the aggregation takes the place of the filter's compaction and of the copy back: orcgpu_reader_d2h_bytes stays 0, one
 * host wait per stripe.  The stripes' records are merged on the host in stripe order (integer and Decimal words added with
 * carry, doubles added in stripe order, flags OR-ed).  orcgpu_reader_filter_rows reports seen and kept rows as under the filter.
 * The projection must hold the aggregated and the filter's columns; whatever else it holds is decoded as always.  On such a
 * reader orcgpu_reader_next_batch[_device] return ORCGPU_INVALID_ARGUMENT and leave it usable; orcgpu_reader_aggregate without
 * aggregates set is ORCGPU_INVALID_ARGUMENT, a second call ORCGPU_END_OF_FILE. */
int orcgpu_reader_set_aggregates(orcgpu_reader* r, const orcgpu_agg_spec* specs, uint32_t n_specs);
int orcgpu_reader_aggregate(orcgpu_reader* r, orcgpu_agg_value* out);
/* ---- GROUP BY for the aggregates: one record per (aggregate, group), the keys hashed on the device ---------------------------
 * TPC-H Q1 is SELECT l_returnflag, l_linestatus, sum(...), count(*) ... GROUP BY l_returnflag, l_linestatus.  The aggregate list
 * above is reduced per GROUP of kept rows (device/agg_group_kernels.hip); what comes back is the groups' keys and one value per
 * (group, aggregate), and nothing else.  The reference has no aggregation; the semantics are fixed here.  By default
 * low-cardinality grouping, at most ORCGPU_GROUP_MAX groups in one result (one stripe) -- flags, statuses, dates, small codes;
 * a higher limit is opt-in (LIMITS below).
 *   - Kept rows and aggregates are what they are above: every op, column kind, refusal and overflow rule, applied per group.
 *     COUNT_ROWS of a group is its kept rows and never 0: a group exists only if a kept row has its key.  (An unconditioned
 *     COUNT_ROWS: under a condition of its own -- FILTER (WHERE ...) below -- it may be 0.)
 *   - KEYS: 1 .. ORCGPU_GROUP_MAX_KEYS key columns, named like the aggregates' columns: projected root columns.  A column may be
 *     a key and an aggregated column.  Byte .. Long, Date (days) and Timestamp / Timestamp-instant decoded to an int64 unit are
 *     ORCGPU_GROUP_KEY_I64 (w[0], sign-extended into w[1]); Boolean is ORCGPU_GROUP_KEY_BOOL (w[0] = 0 / 1); Decimal is
 *     ORCGPU_GROUP_KEY_DEC128, compared as the unscaled 128-bit value (one column has one scale); String / Varchar / Char are
 *     ORCGPU_GROUP_KEY_STRING (the name ORCGPU_GROUP_KEY_BYTES is the limit below), compared as the exported bytes (a Char value includes its padding), len bytes in `bytes`.
 *     scale_or_unit: the Decimal scale, a Timestamp's unit (0 s .. 3 ns), else -1.
 *   - Refused, the message naming the column: a Float / Double or Binary key ORCGPU_MISMATCHED_SCHEMA; a key column read as a
 *     dictionary column, a Timestamp key decoded to Decimal128(38, 9), a nested column in the result ORCGPU_UNSUPPORTED; an unknown
 *     column, a key listed twice, no key, more than ORCGPU_GROUP_MAX_KEYS keys ORCGPU_INVALID_ARGUMENT.
 *   - A NULL key value is a key value of its own, as in SQL: the rows whose key is NULL in that column and equal in the others
 *     form one group, reported with is_null = 1 (and everything else of that key 0).
 *   - Data-dependent limits, found on the device and reported after the call's one wait as ORCGPU_UNSUPPORTED, nothing returned:
 *     more than ORCGPU_GROUP_MAX groups in one result (the message gives the limit); a String key value of more than
 *     ORCGPU_GROUP_KEY_BYTES bytes among the kept rows (the message names the column).  For the reader also a total of more than
 *     ORCGPU_GROUP_MAX_TOTAL groups over all stripes.
 *   - ORDER: groups come back in order of first appearance -- by the smallest kept input row of the group within a result, by
 *     stripe order across stripes.  The whole answer is the same on every run of the same call: groups, order, integer and Decimal
 *     values (exact), MIN / MAX, and Float / Double sums bit for bit (a reduction of fixed shape; no floating-point atomic; which
 *     thread wins a race for a slot of the hash table shows in no output).
 *   - No kept row: zero groups, not one group of NULLs.
 *   - LIMITS.  ORCGPU_GROUP_MAX and ORCGPU_GROUP_MAX_TOTAL are the defaults.  orcgpu_reader_set_group_limits and
 *     orcgpu_result_aggregate_groups_limit (below) raise them, up to ORCGPU_GROUP_LIMIT_MAX groups in one result and
 *     ORCGPU_GROUP_TOTAL_LIMIT_MAX over a reader's stripes -- GROUP BY l_suppkey, l_partkey, l_orderkey.  Everything above holds per
 *     group with only the numbers changed: the data-dependent refusals are "more than max_groups groups in one result" and "more
 *     than max_total groups over the stripes", ORCGPU_UNSUPPORTED, the message giving the limit that was set.
 *     WHICH PATH RUNS is decided by the limit alone, on the host, never by the data: max_groups <= ORCGPU_GROUP_MAX runs the
 *     reduction described above (accumulators per group in LDS); a higher limit runs, for the whole call and however few groups
 *     the rows hold, the wide path (device/agg_group_wide_kernels.hip): the kept rows are sorted stably by their group's number of
 *     first appearance (an LSD radix sort, 8 bits a pass, as many passes as the limit needs) and every group is reduced as one
 *     segment, its rows in ascending input-row order, in a tree whose shape depends on the group's kept-row count alone.  Its cost
 *     follows the rows, not the limit; its device workspace holds records for min(max_groups, input rows) groups.  Integers,
 *     Decimals, MIN / MAX, groups and order are the same on both paths; a Float / Double sum may differ in its last bits between
 *     the two, because the order of summation differs.  Each path is deterministic for itself: on the wide path the whole answer,
 *     Float sums bit for bit, is a function of the kept rows in input order and of max_groups only.
 *     HOST WAITS: the narrow path one per call, as above.  The wide path TWO: the first fetches the group count and the flags
 *     (16 bytes), and -- the flags checked -- the second exactly n_groups key records and n_groups x aggregates value records.
 *     Nothing copied back is sized by the limit. */
#define ORCGPU_GROUP_MAX_KEYS 4
#define ORCGPU_GROUP_MAX 256
#define ORCGPU_GROUP_MAX_TOTAL 65536
#define ORCGPU_GROUP_LIMIT_MAX 1048576
#define ORCGPU_GROUP_TOTAL_LIMIT_MAX 16777216
#define ORCGPU_GROUP_KEY_BYTES 64
enum { ORCGPU_GROUP_KEY_I64 = 0, ORCGPU_GROUP_KEY_DEC128 = 1, ORCGPU_GROUP_KEY_BOOL = 2, ORCGPU_GROUP_KEY_STRING = 3 };
typedef struct {
  uint32_t kind;        /* ORCGPU_GROUP_KEY_I64 / _DEC128 / _BOOL / _BYTES_KIND */
  uint32_t is_null;
  int32_t scale_or_unit;
  uint32_t len;         /* bytes of a String key */
  uint64_t w[2];        /* little-endian words, two's complement */
  uint8_t bytes[ORCGPU_GROUP_KEY_BYTES];
} orcgpu_group_key;
typedef struct orcgpu_groups orcgpu_groups;
/* orcgpu_result_aggregate with a GROUP BY: the rows of `r` the predicate keeps, grouped by key_columns, every group reduced by
 * specs.  *out is a handle to free with orcgpu_groups_free (NULL on failure).  The result is read and left as it was; one host
 * wait per call, which fetches the group count, the flags, the key records and the value records. */
int orcgpu_result_aggregate_groups(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                   const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                   const orcgpu_agg_spec* specs, uint32_t n_specs, orcgpu_groups** out);
/* A builder setter beside orcgpu_reader_set_aggregates (before the first call; the names are copied): the reader's aggregates
 * are grouped.  orcgpu_reader_aggregate_groups drains it as orcgpu_reader_aggregate does: per stripe the grouped aggregation stands
 * where the ungrouped one stands, orcgpu_reader_d2h_bytes stays 0, orcgpu_reader_filter_rows reports as under the filter; the
 * stripes' groups are merged on the host by key in first-appearance order.  orcgpu_reader_aggregate on a reader with a group-by
 * set, and orcgpu_reader_aggregate_groups on one without, are ORCGPU_INVALID_ARGUMENT and leave the reader usable; a group-by
 * without aggregates is ORCGPU_INVALID_ARGUMENT at the drain; a second drain is ORCGPU_END_OF_FILE.
 * ORCGPU_GROUP_HASH_BITS=N (1 .. 32, read per call) keeps N bits of the key tuples' hash, for tests of long probe sequences: the
 * answer is the same. */
int orcgpu_reader_set_group_by(orcgpu_reader* r, const char* const* key_columns, uint32_t n_keys);
int orcgpu_reader_aggregate_groups(orcgpu_reader* r, orcgpu_groups** out);
/* ---- SUM and AVG over arithmetic expressions, evaluated per kept row on the device --------------------------------------------
 * TPC-H Q1's select list holds sum(l_extendedprice * (1 - l_discount)), sum(l_extendedprice * (1 - l_discount) * (1 + l_tax)) and
 * three averages.  One aggregate argument may be an arithmetic EXPRESSION over columns and literals, evaluated exactly, per kept
 * row, in kernels beside those that reduce the plain aggregates (device/agg_expr_eval.h, device/agg_kernels.hip).  The reference has
 * no aggregation; the semantics are fixed here.
 *   - NODES, in pre-order like orcgpu_predicate_node: ORCGPU_AGG_EXPR_COLUMN (`column`: a projected root column),
 *     ORCGPU_AGG_EXPR_LITERAL (value_type ORCGPU_PV_INT64: i; ORCGPU_PV_FLOAT64: f; ORCGPU_PV_DECIMAL128: s / s_len / i under the
 *     rules of that value type in predicates), ORCGPU_AGG_EXPR_ADD / _SUB / _MUL (exactly two children) and ORCGPU_AGG_EXPR_NEG (one).
 *     ORCGPU_AGG_EXPR_DATE_PART (one child, the part in `i`) is the one function: DATE PARTS below.
 *     ORCGPU_AGG_EXPR_DIV / _FLOOR_DIV / _MOD (exactly two children; DIV: a result scale in `i`): DIVISION below.
 *     ORCGPU_AGG_EXPR_IF / _COALESCE / _ABS / _NULL and the condition nodes _CMP / _IS_NULL / _AND / _OR / _NOT: CONDITIONALS below.
 *     ORCGPU_AGG_EXPR_CAST / _ROUND / _FLOOR / _CEIL / _TRUNC (one child each): CONVERSIONS below.
 *   - CLASSES, decided bottom-up when the list is compiled:
 *       INT    Byte .. Long columns and INT64 literals.  Every intermediate value is a signed 128-bit integer.  ORCGPU_AGG_KIND_I128.
 *       DEC    at least one Decimal column or DECIMAL128 literal; Byte .. Long columns and INT64 literals beside them count as
 *              Decimals of scale 0.  a * b has the scale s_a + s_b; a + b and a - b the scale max(s_a, s_b), the operand of lower
 *              scale multiplied by the power of ten, exactly; NEG keeps the scale.  A node whose scale passes 38:
 *              ORCGPU_UNSUPPORTED, the message names the expression's first column.  Every intermediate value is the unscaled
 *              signed 128-bit integer.  ORCGPU_AGG_KIND_DEC128 at the root's scale; overflow = 1 when the final |sum| >= 10^38.
 *       FLOAT  Float / Double columns (a Float widened first) and FLOAT64 literals; INT64 literals too when (double)i is exact,
 *              else ORCGPU_INVALID_ARGUMENT.  Every operation is ONE IEEE double operation rounded once: nothing is contracted into
 *              a fused multiply-add.  ORCGPU_AGG_KIND_F64, deterministic as SUM is: the same bits on every run of the same call.
 *   - REFUSED when the list is compiled.  ORCGPU_MISMATCHED_SCHEMA, the message naming the column: a Float / Double column or a
 *     FLOAT64 literal together with an integer or Decimal column; a FLOAT64 literal in an INT / DEC expression (a DECIMAL128
 *     literal in a FLOAT one); a column of any other kind (Date, Boolean, Timestamp, String, ...).  ORCGPU_UNSUPPORTED: a column read
 *     as a dictionary column, a Timestamp decoded to Decimal128 (as for SUM); an expression that needs more than
 *     ORCGPU_AGG_EXPR_MAX_DEPTH operand slots when the child that needs more slots is evaluated first (of the trees of
 *     ORCGPU_AGG_EXPR_MAX_NODES nodes only the perfectly balanced one of 16 leaves does; operand order never changes a result).
 *     ORCGPU_INVALID_ARGUMENT: an unknown or unprojected column; a malformed tree (a wrong child count -- n_children is not
 *     carried: an operator simply takes the nodes behind it --, nodes left over, an unknown node op, a literal of another value
 *     type, a bad Decimal literal); an expression without any column; more than ORCGPU_AGG_EXPR_MAX_NODES nodes.
 *   - NULLS: a row in which any column of the expression is NULL contributes nothing: the expression is NULL and SUM skips it.
 *   - OVERFLOW: an INT / DEC operation whose exact result does not fit a signed 128-bit integer -- the multiplication by a power of
 *     ten that aligns two scales included -- sets the sticky overflow flag of the aggregate; that row's value is left out, the row
 *     still counts.  Nothing wraps silently.  The sum itself is 192 bits wide, as for SUM.
 *   - DATE PARTS: ORCGPU_AGG_EXPR_DATE_PART takes ONE operand expression and, in `i`, a part: ORCGPU_DATE_PART_YEAR, _QUARTER
 *     (1 .. 4), _MONTH (1 .. 12), _DAY (1 .. 31), _DAY_OF_WEEK (ISO: Monday = 1 .. Sunday = 7), _DAY_OF_YEAR (1 .. 366) -- SQL's
 *     extract(part from date).  The operand's value is an exact integer number of days since 1970-01-01; the calendar is the
 *     proleptic Gregorian one with astronomical year numbering (year 0 exists, the years before it are negative), as numpy's
 *     datetime64 and Arrow's date32 kernels count.  In every stage that speaks this language -- the aggregates here, the row
 *     filter's ORCGPU_PRED_CMP_EXPR (there the node is ORCGPU_PRED_EXPR_DATE_PART), the computed columns:
 *       OPERAND  every leaf below the node is a Byte / Short / Int / Long / Date column or an INT64 literal, combined with + - *,
 *                unary - and further date parts.  Below the node a Date column takes part as int64 days in EVERY mode -- outside
 *                it nothing changes: SUM(date + 1) stays ORCGPU_MISMATCHED_SCHEMA.  A Decimal or Float / Double column, or a
 *                DECIMAL128 / FLOAT64 literal, below the node is ORCGPU_MISMATCHED_SCHEMA, the message naming the function
 *                (`year()`, ...) and the column; every other column keeps the refusal it has without the node.
 *       RESULT   an integer: of the INT class, or of scale 0 inside a DEC expression (year(d) * 100 + month(d), year(d) * price).
 *                A FLOAT expression does not take the node: ORCGPU_MISMATCHED_SCHEMA.
 *       RANGE    the operand must lie in int32, what a Date column holds (years -5877641 .. 5881580).  Outside it the row
 *                OVERFLOWS exactly as an operation that leaves 128 bits does (below; UNKNOWN and counted in the row filter, NULL and
 *                counted in a computed column): never a wrapped or clamped value.
 *       NULL     where any column of the operand is NULL, like every other node.  A date part of literals alone is folded when the
 *                list is compiled, unless it overflows: then it is left to the rows.
 *       LIMITS   the node counts against ORCGPU_AGG_EXPR_MAX_NODES and needs the operand slots of its operand.  A part outside
 *                0 .. 5 and a node without its operand are ORCGPU_INVALID_ARGUMENT.
 *     Row-group pruning does not look through the node: a filter leaf that holds one keeps every row group.
 *   - DIVISION: three binary nodes, a / b (ORCGPU_AGG_EXPR_DIV), a // b (_FLOOR_DIV) and a % b (_MOD), in every stage that speaks
 *     this language -- the aggregates here, the row filter's ORCGPU_PRED_CMP_EXPR (there the nodes are ORCGPU_PRED_EXPR_DIV /
 *     _FLOOR_DIV / _MOD), the computed columns:
 *       a / b, FLOAT   one IEEE double division, correctly rounded: x / 0 is +-Infinity and 0 / 0 NaN.  Never an overflow.  `i` is
 *                not read beyond its range check.
 *       a / b, EXACT   an expression of integer or Decimal leaves that holds a `/` ANYWHERE is of the DEC class, with no Decimal leaf
 *                at all too: long / 2 is a Decimal.  With the operands' scales sa and sb, the result's scale s is the node's `i`:
 *                0 .. 38 the caller's choice, -1 the default rule s = min(38, max(6, sa + 4)); any other `i` is
 *                ORCGPU_INVALID_ARGUMENT.  Let k = s - sa + sb: k < 0 or k > 38 is ORCGPU_UNSUPPORTED, the message naming the three
 *                scales.  The value is the exact quotient at scale s, rounded half away from zero as AVG's is: over the unscaled
 *                integers Q = round(A * 10^k / B).  The row OVERFLOWS when B = 0, when A * 10^k leaves a signed 128-bit integer, or
 *                when the quotient does (-2^127 / -1).  A 256-bit numerator, which would keep the rows whose quotient fits although
 *                A * 10^k does not, is not built: those rows overflow.
 *       a // b, a % b  Python's and numpy's rule: the quotient is floored and the remainder has the divisor's sign, so that
 *                a == (a // b) * b + a % b.  Both operands are integers: of the INT class, or subtrees of scale 0 inside a DEC
 *                expression (year(d) % 100 beside a price); the result is an integer, of scale 0.  An operand of a non-zero scale is
 *                ORCGPU_MISMATCHED_SCHEMA, the message naming the operator and the expression's first column; either operator in a
 *                FLOAT expression is the same status.  The row OVERFLOWS when b = 0, and for // at -2^127 // -1.  An INT
 *                expression that holds only these two stays of the INT class.
 *       OVERFLOW is what it is everywhere in this language: AGG_OVERFLOW's sticky flag in an aggregate, UNKNOWN and counted in the
 *                row filter, NULL and counted in a computed column.  A result is never wrapped, clamped or silently NULL.
 *       NULL     where any column of either operand is NULL.  A division of literals alone is folded when the list is compiled,
 *                unless it overflows: then it is left to the rows.
 *       LIMITS   each node counts against ORCGPU_AGG_EXPR_MAX_NODES and needs operand slots like + - *.  The operand of a date part
 *                is an integer: a quotient of a non-zero scale below one is ORCGPU_MISMATCHED_SCHEMA.
 *     Row-group pruning does not look through a division: a filter leaf that holds one keeps every row group.
 *   - CONDITIONALS: nine nodes, in every stage that speaks this language (in the row filter's ORCGPU_PRED_CMP_EXPR they are
 *     ORCGPU_PRED_EXPR_IF .. _NOT, 20 further on).  Four produce a NUMBER:
 *       IF(cond, a, b)  three children.  a where cond is TRUE, b where it is FALSE or UNKNOWN (SQL's CASE WHEN cond THEN a ELSE b END;
 *                nest it for more branches).
 *       COALESCE(a, b)  two children.  a unless a is NULL, then b.
 *       ABS(a)   one child.  -2^127 overflows; on doubles the sign bit is cleared (abs(-0.0) = 0.0, a NaN keeps its payload).
 *       NULL     no children.  It takes the class and scale of the sibling it meets as a value operand of IF or COALESCE; anywhere
 *                else, and beside another NULL, it is ORCGPU_INVALID_ARGUMENT.
 *     and five produce a CONDITION -- TRUE, FALSE or UNKNOWN --, legal only as the first child of IF or below AND / OR / NOT:
 *       CMP(a, b)  `i` holds ORCGPU_PRED_EQ .. _GE (anything else: ORCGPU_INVALID_ARGUMENT).  UNKNOWN where either side is NULL.
 *                Integers and Decimals compare exactly, the side of the smaller scale first brought to the larger as + brings it
 *                (times a power of ten, which can overflow that side).  Doubles compare by IEEE's rules: with a NaN every
 *                comparison is FALSE but !=.
 *       IS_NULL(a)  TRUE or FALSE, never UNKNOWN.
 *       AND, OR, NOT  Kleene's.
 *     A condition where a number is wanted, or a number where a condition is wanted -- the root of an expression is a number --, is
 *     ORCGPU_INVALID_ARGUMENT, the message naming the node.
 *       CLASSES  the two value operands of IF and of COALESCE, and the two sides of CMP, are of one class: an integer beside a
 *                Decimal is promoted as + promotes it, a Float / Double beside an integer or Decimal is refused as + refuses it
 *                (ORCGPU_MISMATCHED_SCHEMA).  The result has the larger of the two scales; the other operand is taken times the power
 *                of ten, which can overflow THAT operand only.
 *       NULL AND OVERFLOW ARE PER OPERAND, not per row.  Every operand has a value, "is NULL" and "overflowed".  Arithmetic (+ - * /
 *                // %, unary -, ABS, a date part, the scale alignment) gives NULL if an operand is NULL -- NULL comes first --,
 *                otherwise overflow if an operand overflowed or the operation does.  CMP the same, with UNKNOWN for NULL.  IS_NULL of
 *                an operand that overflowed overflows.  IF takes the three fields of the branch it chooses: the other branch may be
 *                NULL, divide by zero or leave 128 bits, and nothing is seen of it; a condition that overflowed overflows the IF.
 *                COALESCE takes a's fields unless a is NULL, then b's: it overflows if a overflowed.  AND and OR are decided by value:
 *                a FALSE operand makes AND FALSE and a TRUE operand makes OR TRUE whatever the other operand is or did, on either
 *                side; otherwise overflow comes before UNKNOWN.  So IF(b != 0, a / b, 0) and IF(b != 0 AND a / b > 2, ..) count no
 *                overflow where b = 0.  NOT keeps UNKNOWN and overflow.  Both branches are evaluated on every row; the fields make
 *                that invisible.
 *       THE ROOT decides the row as it always did: overflow is AGG_OVERFLOW in an aggregate, UNKNOWN and counted in the row filter,
 *                NULL and counted in a computed column; NULL is a row that contributes nothing, UNKNOWN, and a NULL that is not
 *                counted.
 *       LIMITS   every node counts against ORCGPU_AGG_EXPR_MAX_NODES.  Operand slots follow the Sethi-Ullman labelling extended to
 *                the ternary node with its condition first: with the labels lc, la, lb of its children, IF needs
 *                max(lc, 1 + (la == lb ? la + 1 : max(la, lb))); more than ORCGPU_AGG_EXPR_MAX_DEPTH is ORCGPU_UNSUPPORTED.
 *                An ABS of a literal is folded; no other conditional node is.  An expression without any column stays
 *                refused where it was.
 *     Row-group pruning does not look through a conditional: a filter leaf that holds one keeps every row group.
 *   - CONVERSIONS: five nodes with one child each, in every stage that speaks this language (in the row filter's
 *     ORCGPU_PRED_CMP_EXPR they are ORCGPU_PRED_EXPR_CAST .. _TRUNC, 20 further on): conversion BETWEEN the classes, and rounding
 *     inside them.  Without one, a Float / Double beside an integer or a Decimal stays ORCGPU_MISMATCHED_SCHEMA (the message says
 *     that a cast brings them together); with one, l_quantity * weight is cast(l_quantity, FLOAT64) * weight.
 *       CLASSES  An expression that holds one of these nodes has its classes decided PER NODE, bottom-up.  The two operands of
 *                + - * / // %, the two sides of CMP and the value operands of IF / COALESCE are still of one class: INT beside DEC
 *                is promoted, an INT64 literal beside doubles is a double where that is exact, doubles beside anything else are
 *                ORCGPU_MISMATCHED_SCHEMA.  a / b of two integers is a Decimal.  CAST gives its subtree the target class; ROUND,
 *                FLOOR, CEIL and TRUNC keep their child's.  The ROOT's class decides the aggregate's kind and the computed column's
 *                type (Int64 / Decimal128(38, s) / Float64).  A date part, // and % keep their integer operands: CAST to INT64 below
 *                them is legal, and so is FLOOR / CEIL / TRUNC / ROUND to 0 digits of a Decimal, which is of scale 0.  What stands
 *                below a conversion is not "below the date part" above it: a Date column there is what it is without the part.
 *       CAST     value_type = the target: ORCGPU_PV_INT64, _FLOAT64 or _DECIMAL128, then i = the scale t, 0 .. 38.
 *                to FLOAT64   from FLOAT: nothing (no op).  From INT, or DEC at scale s: the double nearest the exact rational
 *                             unscaled / 10^s, ties to even -- Python's float(Fraction(unscaled, 10**s)).  Never an overflow.
 *                to DECIMAL128 at scale t   from INT, or DEC at scale s <= t: times 10^(t - s), checked.  From DEC at scale s > t:
 *                             divided by 10^(s - t), rounded half away from zero (AVG's and /'s rule).  From FLOAT: the double's
 *                             exact value m * 2^e times 10^t, computed exactly and rounded half away from zero; NaN, an infinity
 *                             and a result of magnitude 10^38 or more overflow the row; -0.0 gives 0.  DEC at scale t.
 *                to INT64     from INT: the value.  From DEC at scale s: the unscaled value divided by 10^s, truncated toward zero.
 *                             From FLOAT: truncated toward zero (Arrow's, Spark's and C's rule; rounding is cast(round(x))).  In all
 *                             three a result outside int64 overflows the row, as do NaN and the infinities.  INT.
 *       ROUND    i = the digits n, 0 .. 38.  DEC at scale s: unchanged where n >= s, else rescaled to scale n, half away from zero.
 *                INT: unchanged.  FLOAT: n must be 0 -- C's round(), half away from zero, still a double; NaN and the infinities
 *                pass --; n > 0 is ORCGPU_UNSUPPORTED (the message: round a double to n places with a cast to DECIMAL128 at n).
 *       FLOOR, CEIL, TRUNC   DEC at scale s: the integer, at scale 0, toward -infinity, toward +infinity, toward zero.  INT: unchanged,
 *                no op.  FLOAT: IEEE floor / ceil / trunc, still a double.
 *       NULL AND OVERFLOW are per operand, as with the CONDITIONALS -- a program with a conversion is laid out and run like one with
 *                a conditional --: NULL in gives NULL out; overflow is the language's: AGG_OVERFLOW in an aggregate (of the FLOAT
 *                class too, where a conversion inside overflowed), UNKNOWN and counted in the row filter, NULL and counted in a
 *                computed column.
 *       LIMITS   every node counts against ORCGPU_AGG_EXPR_MAX_NODES and needs the operand slots of its child.  A conversion of a
 *                literal alone is folded when the list is compiled, unless it overflows: then it is left to the rows.
 *       REFUSED  ORCGPU_INVALID_ARGUMENT: a CAST whose value_type is no target, a scale or digits outside 0 .. 38, a node without
 *                its child, a condition as the child (the message names the node).  ORCGPU_UNSUPPORTED: ROUND of a double to n > 0.
 *     Row-group pruning does not look through a conversion: a filter leaf that holds one keeps every row group.
 *   - OPS: ORCGPU_AGG_OP_SUM_EXPR the sum of the expression over the kept rows where it is not NULL, NULL over no such row;
 *     ORCGPU_AGG_OP_AVG the average of a plain column (the columns SUM takes); ORCGPU_AGG_OP_AVG_EXPR the average of an expression.
 *     A *_EXPR op without an expression -- through an entry point without `exprs` too -- is ORCGPU_INVALID_ARGUMENT.
 *   - AVG is the exact sum divided by the number of values, finished on the host.  FLOAT: sum / (double)count.  INT:
 *     ORCGPU_AGG_KIND_F64, the double nearest to the exact rational sum / count, ties to even; a sum that does not fit 128 bits is
 *     overflow = 1.  DEC at scale s: ORCGPU_AGG_KIND_DEC128 at scale min(s + 4, 38), the exact quotient rounded half away from zero
 *     (Hive's and Spark's rule); overflow = 1 when the sum overflowed or |result| >= 10^38.  Over no value: NULL.
 * The three entry points below are the ones above with a second array parallel to `specs`: exprs[k] is the expression of specs[k],
 * {NULL, 0} for an op that takes none (exprs = NULL: no spec has one -- this is what the entry points above call).  Everything said
 * of the aggregates holds per expression aggregate: row selection, filter, pruning, grouping, the merge across stripes, no byte
 * copied back, one wait per stripe.  orcgpu_reader_set_aggregate_exprs copies nodes, names and literal bytes;
 * orcgpu_reader_aggregate[_groups] drain as before. */
#define ORCGPU_AGG_EXPR_MAX_NODES 32
#define ORCGPU_AGG_EXPR_MAX_DEPTH 4
enum { ORCGPU_AGG_OP_SUM_EXPR = 6, ORCGPU_AGG_OP_AVG = 7, ORCGPU_AGG_OP_AVG_EXPR = 8 };
enum { ORCGPU_AGG_EXPR_COLUMN = 0, ORCGPU_AGG_EXPR_LITERAL = 1, ORCGPU_AGG_EXPR_ADD = 2, ORCGPU_AGG_EXPR_SUB = 3, ORCGPU_AGG_EXPR_MUL = 4,
       ORCGPU_AGG_EXPR_NEG = 5,
       /* (6 .. 15: unknown nodes) */
       ORCGPU_AGG_EXPR_DATE_PART = 16 /* one child; i = ORCGPU_DATE_PART_*: see DATE PARTS above */,
       ORCGPU_AGG_EXPR_DIV = 17 /* a / b; i = the result scale 0 .. 38 of an exact division, -1: the default rule */,
       ORCGPU_AGG_EXPR_FLOOR_DIV = 18 /* a // b */, ORCGPU_AGG_EXPR_MOD = 19 /* a % b: two children each; see DIVISION above */,
       /* (20: an unknown node).  CONDITIONALS above -- value nodes: */
       ORCGPU_AGG_EXPR_IF = 21 /* three children: a condition, then, otherwise */, ORCGPU_AGG_EXPR_COALESCE = 22 /* two children */,
       ORCGPU_AGG_EXPR_ABS = 23 /* one child */, ORCGPU_AGG_EXPR_NULL = 24 /* no children: the NULL of its sibling's class and scale */,
       /* ... and condition nodes, legal only as the first child of IF or below AND / OR / NOT: */
       ORCGPU_AGG_EXPR_CMP = 25 /* two value children; i = ORCGPU_PRED_EQ .. _GE (0 .. 5) */, ORCGPU_AGG_EXPR_IS_NULL = 26 /* one value child */,
       ORCGPU_AGG_EXPR_AND = 27, ORCGPU_AGG_EXPR_OR = 28 /* two condition children */, ORCGPU_AGG_EXPR_NOT = 29 /* one condition child */,
       /* CONVERSIONS above: one child each */
       ORCGPU_AGG_EXPR_CAST = 30 /* value_type = the target ORCGPU_PV_INT64 / _FLOAT64 / _DECIMAL128; DECIMAL128: i = the scale 0 .. 38 */,
       ORCGPU_AGG_EXPR_ROUND = 31 /* i = the digits 0 .. 38 */, ORCGPU_AGG_EXPR_FLOOR = 32, ORCGPU_AGG_EXPR_CEIL = 33, ORCGPU_AGG_EXPR_TRUNC = 34 };
enum { ORCGPU_DATE_PART_YEAR = 0, ORCGPU_DATE_PART_QUARTER = 1, ORCGPU_DATE_PART_MONTH = 2, ORCGPU_DATE_PART_DAY = 3,
       ORCGPU_DATE_PART_DAY_OF_WEEK = 4, ORCGPU_DATE_PART_DAY_OF_YEAR = 5 };
typedef struct {
  uint32_t op;           /* ORCGPU_AGG_EXPR_*                                   */
  const char* column;    /* COLUMN: the name of a projected root column        */
  int32_t value_type;    /* LITERAL: ORCGPU_PV_INT64 / _FLOAT64 / _DECIMAL128  */
  int64_t i;
  double f;
  const char* s;
  uint64_t s_len;
} orcgpu_agg_expr_node;  /* pre-order, like orcgpu_predicate_node */
typedef struct {
  const orcgpu_agg_expr_node* nodes;
  uint32_t n_nodes;
} orcgpu_agg_expr;
int orcgpu_result_aggregate_exprs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                  const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs,
                                  const orcgpu_agg_expr* exprs, uint32_t n_specs, orcgpu_agg_value* out);
int orcgpu_result_aggregate_groups_exprs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                         const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                         const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, orcgpu_groups** out);
int orcgpu_reader_set_aggregate_exprs(orcgpu_reader* r, const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs);
/* The limits of a GROUP BY (LIMITS above).  orcgpu_result_aggregate_groups_limit is orcgpu_result_aggregate_groups_exprs with the
 * limit of groups in the result: 0 = ORCGPU_GROUP_MAX, a value above ORCGPU_GROUP_LIMIT_MAX ORCGPU_INVALID_ARGUMENT; the entries
 * without a limit are this one called with 0.  orcgpu_reader_set_group_limits is legal where orcgpu_reader_set_group_by is (before
 * the first call, in either order with it): max_groups per stripe and max_total over the stripes, 0 = leave the default (256 /
 * 65536); a value above its maximum, and max_total < max_groups after the defaults are applied, are ORCGPU_INVALID_ARGUMENT and
 * change nothing.  A limit above ORCGPU_GROUP_MAX costs two host waits a stripe instead of one. */
int orcgpu_result_aggregate_groups_limit(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                         const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                         const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, uint32_t max_groups,
                                         orcgpu_groups** out);
int orcgpu_reader_set_group_limits(orcgpu_reader* r, uint32_t max_groups, uint32_t max_total);
/* ---- FILTER (WHERE ...) per aggregate: several aggregates in one pass, each over its own subset of the kept rows ------------------
 * TPC-H Q14 is sum(case when p_type like 'PROMO%' then l_extendedprice * (1 - l_discount) else 0 end) beside the same sum over
 * every row; Q12 counts two priority classes side by side; every pivot is this shape.  In SQL: agg(x) FILTER (WHERE p), or
 * agg(CASE WHEN p THEN x END).  An aggregate may carry a CONDITION, evaluated per row on the device (agg_cond_eval_kernel in
 * device/agg_kernels.hip, with the row filter's own per-word evaluation) in front of the kernels that reduce.  The reference has no
 * aggregation; the semantics are fixed here.
 *   - A condition is a predicate in exactly the row filter's language (orcgpu_result_filter above): the same nodes in pre-order,
 *     the same literal rules, the same three-valued logic, ORCGPU_FILTER_MAX_DEPTH per condition, and the same refusals with the
 *     same statuses and messages (they begin "row filter:").  Its leaves name projected root columns.
 *   - THE RULE: a conditioned aggregate is the same aggregate computed as if its argument were NULL in every kept row for which
 *     the condition is not TRUE -- FALSE and UNKNOWN alike.  Everything else follows: COUNT_ROWS with a condition counts the kept
 *     rows where it is TRUE, COUNT(c) those of them where c is not null; SUM, MIN, MAX, SUM_PRODUCT, SUM_EXPR, AVG and AVG_EXPR
 *     skip the other rows exactly as they skip NULL values -- NULL over no passing value, AVG divides by the passing values, the
 *     sticky overflow flag is set by passing rows only.
 *   - The KEPT rows are what they were: row selection and row filter.  Conditions change neither them nor
 *     orcgpu_reader_filter_rows, prune no row groups and change no stripe planning.  A GROUP exists iff a kept row has its key,
 *     whatever the conditions say, and the order stays first appearance among the kept rows; a group in which no row passes an
 *     aggregate's condition reports that aggregate as NULL, or 0 for the counts.  So "COUNT_ROWS of a group is never 0" (GROUP BY
 *     above) holds for an unconditioned COUNT_ROWS only.
 *   - DETERMINISM: a row that does not pass adds nothing to a Float / Double sum -- it is left out, it does not add +0.0 -- and the
 *     shape of every reduction stays the function it was: the ungrouped grid of the input row count, the wide path's fold of the
 *     group's kept-row count c and of every row's lane, a row that does not pass being a lane step that adds nothing.  The same
 *     call gives the same bits.  Ungrouped, aggregate(a FILTER (WHERE p)) under the row filter f is, bit for bit, aggregate(a)
 *     under f AND p.
 *   - LIMITS: conditions that are node for node the same (op, children, column, literal kind and bytes) share one evaluation; at
 *     most ORCGPU_AGG_MAX distinct conditions a list.  The device workspace holds one mask plane (one bit per input row) per
 *     distinct condition; what cannot be had is the aggregation's out-of-memory status.  No further host wait.
 *   - Not there: CASE with a non-NULL ELSE inside an arithmetic expression; conditions as pruning predicates.
 * The entry points below are the ones above with a third array parallel to `specs`: filters[k] is the condition of specs[k],
 * {NULL, 0} for none -- n_nodes = 0 is "none" at every entry point, whatever `nodes` holds; a count without nodes is
 * ORCGPU_INVALID_ARGUMENT -- (filters = NULL: no spec has one -- this is what every entry point above calls; exprs may be NULL likewise).
 * orcgpu_result_aggregate_groups_filters takes max_groups as orcgpu_result_aggregate_groups_limit does (0: ORCGPU_GROUP_MAX).
 * orcgpu_reader_set_aggregate_filters is legal after orcgpu_reader_set_aggregates[_exprs] and before the first call; it copies
 * nodes, names and literal bytes; n_specs must be the list's, else ORCGPU_INVALID_ARGUMENT and nothing changes; a later
 * orcgpu_reader_set_aggregates[_exprs] drops the conditions with the list they belonged to. */
typedef struct {
  const orcgpu_predicate_node* nodes;  /* pre-order, as for orcgpu_result_filter */
  uint32_t n_nodes;
} orcgpu_agg_filter;
int orcgpu_result_aggregate_filters(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                    const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs,
                                    const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters, uint32_t n_specs, orcgpu_agg_value* out);
int orcgpu_result_aggregate_groups_filters(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                           const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                           const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters,
                                           uint32_t n_specs, uint32_t max_groups, orcgpu_groups** out);
int orcgpu_reader_set_aggregate_filters(orcgpu_reader* r, const orcgpu_agg_filter* filters, uint32_t n_specs);
uint32_t orcgpu_groups_count(const orcgpu_groups* g);
int orcgpu_groups_key(const orcgpu_groups* g, uint32_t group, uint32_t key, orcgpu_group_key* out);
int orcgpu_groups_value(const orcgpu_groups* g, uint32_t group, uint32_t spec, orcgpu_agg_value* out);
void orcgpu_groups_free(orcgpu_groups* g);
/* ---- Top-k: ORDER BY ... LIMIT k, the top rows selected on the device -------------------------------------------------------------
 * SELECT ... WHERE ... ORDER BY x [DESC] LIMIT k: the ten largest orders, the hundred latest events.  The aggregates return one
 * record, the row filter every kept row; this returns the k first kept rows under a sort order, chosen and ordered where the rows
 * lie (device/top_k_kernels.hip: a radix select over the key bytes, then a stable radix sort of at most k rows), so that only they
 * cross the link.  The reference has no ORDER BY and no LIMIT; the semantics are fixed here.
 *   - The KEPT rows are what they are for the row filter and the aggregates: those the row selection selects (if there is one) for
 *     which the row filter's root is TRUE (if there is one); with neither, every row.
 *   - SORT KEYS: 1 .. ORCGPU_TOP_K_MAX_KEYS, the first the most significant; each names a projected root column.  Byte .. Long,
 *     Date (days) and a Timestamp / Timestamp-instant decoded to an int64 unit compare as signed 64-bit integers; Boolean false <
 *     true; Decimal as the unscaled signed 128-bit value (one column has one scale); Float / Double as double, a Float widened
 *     first, in the total order -inf < finite < +inf < NaN, every NaN equal to every other, -0.0 equal to 0.0.
 *   - PER-KEY FLAGS: `descending` reverses the order of that key's non-null values only; `nulls_first` places its NULLs before
 *     all of its non-null values, whatever `descending` says -- the default is after them.
 *   - THE ANSWER: the kept rows sorted STABLY by the keys -- rows equal in every key keep ascending input-row order, which across
 *     stripes is stripe order, then row --, the first k of them.  Ties included it is a function of the kept rows in input order,
 *     the keys and k: the same on every run, whichever thread wins whichever race (no atomic decides a value, a place or an order).
 *   - k: 1 .. ORCGPU_TOP_K_MAX.  Fewer than k kept rows: all of them.  No kept row: no batch.
 *   - Every column of the projection comes along: Strings, Binary, Decimal, Timestamps and dictionary-output columns travel as
 *     payload exactly as the row filter's gather moves them.
 *   - REFUSED, each message beginning "top-k:" and naming the column.  ORCGPU_UNSUPPORTED: a String / Varchar / Char / Binary key; a
 *     key column read as a dictionary column; a Timestamp key decoded to Decimal128(38, 9); a nested column in the result, as for
 *     the filter.  ORCGPU_INVALID_ARGUMENT: an unknown or unprojected column; a key listed twice; no key or more than
 *     ORCGPU_TOP_K_MAX_KEYS; k = 0 or k > ORCGPU_TOP_K_MAX.
 *   - COST: one host wait per call, as for the filter; beside the filter's counters it fetches the select's state and at most k
 *     key records (9 bytes a key, 17 for a Decimal key, rounded up to 8).  The launch sequence is a function of the key kinds and
 *     k alone.  The device workspace holds three planes of one bit per input row, a second row list and the records, behind the
 *     filter's own.
 *   - Not there: String keys (the next step); keys that are expressions; a running cut-off handed from stripe to stripe; OFFSET;
 *     ORDER BY over GROUP BY results.
 * orcgpu_result_top_k is orcgpu_result_filter with ORDER BY keys LIMIT k; n_nodes = 0 is "no predicate".  Afterwards the result's
 * batches are the answer's rows IN SORTED ORDER, packed into batches of batch_size rows, and everything that speaks of a filtered
 * result speaks of them (_rows, _batches, _batch_view, _copy_batch, _fetch[_async], _export_batch[_device]); a copy back moves
 * those rows only.  A result whose status is not OK is left alone and that status returned.  *rows_kept: the rows the predicate
 * kept; *rows_out: min(k, kept).
 * orcgpu_reader_set_top_k is a builder setter (before the first call; names are copied).  Per stripe the top-k stands where the
 * filter's compaction stands -- after the row selection and the row filter if set, with and without read-ahead and device output --:
 * a stripe hands out its own at most k best rows, sorted, in batches of batch_size rows; a stripe without kept rows yields no
 * batch.  orcgpu_reader_filter_rows reports seen and predicate-kept rows, not k.  Together with aggregates it is
 * ORCGPU_INVALID_ARGUMENT at whichever setter comes second, and nothing changes.
 * orcgpu_reader_top_k_order is legal once next_batch[_device] has returned ORCGPU_END_OF_FILE; before that, and on a reader without
 * top-k, it is ORCGPU_INVALID_ARGUMENT.  positions[i] is the index of the i-th row of the GLOBAL answer in the concatenation of all
 * rows the reader handed out, in hand-out order; *n = min(k, total kept rows); cap < *n is ORCGPU_INVALID_ARGUMENT with *n set.
 * (The reader keeps one key record per handed-out row, fetched in the stripe's one wait, and merges them k-way on the host: ties
 * by stripe order, then position.) */
#define ORCGPU_TOP_K_MAX_KEYS 4
#define ORCGPU_TOP_K_MAX 65536
typedef struct {
  const char* column;
  uint32_t descending;   /* 0: ascending */
  uint32_t nulls_first;  /* 0: NULLs behind every value of this key */
} orcgpu_sort_key;
int orcgpu_result_top_k(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                        const char* const* column_names, uint32_t n_columns, const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k,
                        uint64_t* rows_kept, uint64_t* rows_out);
int orcgpu_reader_set_top_k(orcgpu_reader* r, const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k);
int orcgpu_reader_top_k_order(orcgpu_reader* r, uint64_t* positions, uint64_t cap, uint64_t* n);

/* ---- key sets: a semi-join filter against a key set built on the GPU (this library's own) ------------------------------------------
 * `A.key IN (SELECT B.key FROM B WHERE ...)`: the rows of A whose key appears among the kept rows of B.  The BUILD side collects
 * the distinct non-NULL keys of one column over the kept rows of one or more reads into a hash set that stays in HBM, and whether
 * any kept row's key was NULL; the PROBE side names the sealed set in a predicate leaf, ORCGPU_PRED_IN_SET.  No key crosses the link.
 *
 *   - orcgpu_key_set_create: capacity is fixed here.  max_keys: 1 .. ORCGPU_KEY_SET_MAX_KEYS (else ORCGPU_INVALID_ARGUMENT); the
 *     table holds the power of two >= 2 x max_keys slots of 8 bytes, at least 64.  Memory that cannot be had: ORCGPU_HIP_ERROR, as
 *     for every buffer of the library.  ORCGPU_KEY_SET_HASH_BITS = N (1 .. 32) in the environment, read by this call, makes the
 *     build and every probe of the set use N bits of a key's hash: long probe chains, the same membership (a testing aid).
 *   - orcgpu_reader_collect_keys drains the reader the way orcgpu_reader_aggregate does: every stripe is decoded, the row selection
 *     and the row filter are applied as a keep mask only, and the kept rows' keys are inserted where they lie -- no compaction, no
 *     gather, no copy back: no batch is produced, orcgpu_reader_d2h_bytes stays 0, and the insert adds no host wait per stripe.
 *     `column`: a projected root column.  Several readers may collect into one set before it is sealed (a build side split over
 *     files).  A reader with aggregates or a top-k, and one that has handed out a batch: ORCGPU_INVALID_ARGUMENT.  A sharded reader
 *     collects its shard's keys only.  orcgpu_result_collect_keys is the same for one hand-decoded result (nodes: the row filter,
 *     n_nodes = 0: none; column_names: one per column of the result), as orcgpu_result_aggregate is to the reader call.
 *   - Key columns, on both sides: Byte, Short, Int, Long and Date, all taken as int64, as an integer comparison takes them.
 *     ORCGPU_UNSUPPORTED, the message naming the column: a Timestamp column (the units and zones of two files need not agree), a
 *     Decimal, Float / Double, Boolean, String / Varchar / Char / Binary column, one read as a dictionary column, a nested one.
 *     ORCGPU_INVALID_ARGUMENT: an unknown or unprojected column; a sealed (or failed) set passed to collect; an unsealed or failed
 *     set, or one of another context, named by a predicate.
 *   - orcgpu_key_set_seal is the build's ONE host wait.  info: the distinct keys, whether a kept row's key was NULL, and the input
 *     rows the collects went through (behind the row selection, in front of the row filter).  More than max_keys distinct keys
 *     arrived: ORCGPU_UNSUPPORTED, the message gives the limit, and the set is unusable from then on (collect and predicates refuse
 *     it; free it).  After a seal the set is read-only; sealing it again returns the same info.
 *   - orcgpu_key_set_id: unique among all sets of the process, hence within the context; 0 for NULL.
 *   - orcgpu_key_set_free: the handle goes now; the set's memory goes when the last reader, result call or plan whose compiled
 *     filter names it is gone -- a reader that filters by a set may be read to its end after the set has been freed.  Free every
 *     set before orcgpu_close.
 *
 * SEMANTICS, in one rule: `x IN SET s` is exactly ORCGPU_PRED_IN over the values the build side's kept rows held, NULLs included.
 * So a NULL row is UNKNOWN; an empty set is FALSE everywhere (UNKNOWN everywhere when all it saw was NULLs); has_null turns every
 * non-match into UNKNOWN, so NOT over such a leaf keeps nothing -- which is what SQL's `IN (subquery)` requires.  The leaf lives
 * in the filter's language: it serves the row filter, an aggregate's FILTER (WHERE ...) and the top-k's filter alike, beside every
 * other leaf.  As a pruning predicate (orcgpu_reader_set_predicate) it is a sound "might match": it keeps every row group and never
 * fails the evaluation.  A program without such a leaf launches exactly what it launched before there were key sets. */
#define ORCGPU_KEY_SET_MAX_KEYS (1u << 26)
typedef struct orcgpu_key_set orcgpu_key_set;
typedef struct {
  uint64_t n_keys;    /* distinct non-NULL keys                                        */
  uint64_t rows_seen; /* input rows of the collects                                    */
  int32_t has_null;   /* a kept row's key was NULL                                     */
  int32_t pad;
} orcgpu_key_set_info;
int orcgpu_key_set_create(orcgpu_ctx* ctx, uint64_t max_keys, orcgpu_key_set** set);
int orcgpu_reader_collect_keys(orcgpu_reader* r, const char* column, orcgpu_key_set* set);
int orcgpu_result_collect_keys(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                               const char* const* column_names, uint32_t n_columns, const char* column, orcgpu_key_set* set);
int orcgpu_key_set_seal(orcgpu_key_set* set, orcgpu_key_set_info* info);
uint64_t orcgpu_key_set_id(const orcgpu_key_set* set);
void orcgpu_key_set_free(orcgpu_key_set* set);
/* Read-ahead: how many decoded stripes the reader may be ahead of the caller (default 2 -- every result set in flight costs a pinned host copy of a stripe --, at most 8; 0 = none: every stripe is
 * read, staged, decoded and copied back inside the orcgpu_reader_next_batch call that needs it).  With read-ahead two threads
 * of the reader work beside the caller: one reads and stages the stripes to come, one decodes the stripes staged so far
 * (several per call when decoding is the slower side) and starts their copies back, while the caller consumes the batches of
 * an earlier stripe (async_arrow_reader.rs:165-280: StreamState::Reading beside the decoding of the current stripe).  The
 * batches are the same either way.  The context must not be used for other calls while such a reader is open. */
int orcgpu_reader_set_prefetch(orcgpu_reader* r, uint32_t stripes);
uint64_t orcgpu_reader_total_rows(const orcgpu_reader* r);                                           /* total_row_count */
uint32_t orcgpu_reader_stripe_count(const orcgpu_reader* r);
uint32_t orcgpu_reader_column_count(orcgpu_reader* r);                                               /* projected flat columns */
const char* orcgpu_reader_column_name(orcgpu_reader* r, uint32_t i);
/* ArrowReader::next: 0 = one RecordBatch exported (struct array, host memory), ORCGPU_END_OF_FILE = no more batches,
 * anything else = the OrcError status of the failing batch (the iterator then ends). */
int orcgpu_reader_next_batch(orcgpu_reader* r, struct ArrowArray* out_array, struct ArrowSchema* out_schema);

/* ---- Computed columns: arithmetic expressions materialised on the device, once per stripe (this library's own) --------------------
 * A reader may be given 1 .. ORCGPU_COMPUTED_MAX computed columns, each {name, expression}, in order.  The expression is an
 * orcgpu_agg_expr over the nodes of the expression aggregates and of the row filter's comparison: column, literal, + - *, unary -,
 * the date part (ORCGPU_AGG_EXPR_DATE_PART: year(d), month(d), ...; an operand outside int32 is NULL and counted, below) and the
 * divisions (ORCGPU_AGG_EXPR_DIV / _FLOOR_DIV / _MOD; a zero divisor is NULL and counted; int / int is a Decimal128(38, 6) column),
 * and the conditionals (ORCGPU_AGG_EXPR_IF .. _NOT: CASE WHEN, COALESCE, ABS; a NULL result is NULL and not counted).
 *   - OPERANDS are projected flat root columns of the file.  Another computed column as an operand is ORCGPU_UNSUPPORTED.  At most
 *     ORCGPU_AGG_EXPR_MAX_NODES nodes and ORCGPU_AGG_EXPR_MAX_DEPTH operand slots.
 *   - TYPING is the expression compiler's, in the mode one side of ORCGPU_PRED_CMP_EXPR takes: a Date takes part as int64 days; the
 *     class is decided over the whole expression.  Integer class: Int64.  Decimal class: Decimal128(38, s), s by the scale rule of
 *     the expression aggregates.  Float class: Float64, one IEEE operation at a time, never contracted.  The compiler's refusals
 *     keep their messages and name the computed column: Boolean, String / Varchar / Char / Binary, Timestamp, dictionary-output and
 *     nested operands, a node scale above 38, an expression without any column.
 *   - NULL: a row's value is NULL where any column operand is NULL.  It is NULL, and COUNTED, where an operation inside the
 *     expression leaves 128 bits, where an Int64 result does not fit int64, and where a Decimal result has a magnitude of 10^38 or
 *     more: never a wrapped value.  orcgpu_reader_computed_overflow_rows gives the count so far: of the selected rows -- all rows
 *     without a row selection --, before the row filter.
 *   - NAMES are non-empty and distinct, and none equals a root column name of the file, projected or not
 *     (ORCGPU_INVALID_ARGUMENT, naming it).  A nested column in the projection beside computed columns is ORCGPU_UNSUPPORTED, by
 *     name.  These refusals, and the expressions', arrive with the first batch (or the aggregate / collect call): the projection is
 *     known once the reader is built.  Setting them after the first batch is ORCGPU_INVALID_ARGUMENT.
 *   - PLACE: the computed columns follow the projected ones, in the order given, as nullable fields -- in the exported schema, in
 *     every batch, and among the names the row filter, the aggregates (arguments, Agg.where, operands of their expressions), GROUP BY
 *     keys (Int64, Decimal), top-k keys and orcgpu_reader_collect_keys (Int64) resolve against.  They come back through the host
 *     path, the device path, a row selection and the row filter's gather like any fixed-width column of the file.
 *   - As a pruning predicate a leaf on a computed column keeps every stripe and row group: the statistics know nothing of it.
 * The columns are evaluated inside the decode call, behind the last kernel that writes an operand and in front of the call's
 * closing copy, which brings their per-batch null counts and the overflow count back with everything else: no wait is added.  A
 * decode call with computed columns runs on one column lane (the operands must be complete on the stream that evaluates).  The
 * reader's row selection on a stripe is fixed before its decode call, so the count can be of the selected rows there.
 * orcgpu_result_compute_columns does the same on a hand-decoded result, before any orcgpu_result_select / _filter on it:
 * column_names names the result's columns (one per column; they are the operands and the names a computed column may not take),
 * the computed columns are appended behind them -- every later result call then takes n more column names --, *overflow_rows gets
 * the count over all rows.  One host wait of its own.  A result whose decode failed is left alone: its status is returned. */
#define ORCGPU_COMPUTED_MAX 8
int orcgpu_reader_set_computed_columns(orcgpu_reader* r, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n);
int orcgpu_result_compute_columns(orcgpu_ctx* ctx, orcgpu_result* result, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n,
                                  const char* const* column_names, uint64_t* overflow_rows);
int orcgpu_reader_computed_overflow_rows(const orcgpu_reader* r, uint64_t* rows);

/* ---- Key maps and lookup columns: a many-to-one equi-join, build-side columns fetched by key on the device (this library's own) ----
 * `SELECT A.*, B.v FROM A LEFT JOIN B ON A.fk = B.key` where B.key is unique -- a foreign key against a unique key, what a star
 * schema needs.  The BUILD side keeps chosen columns beside its keys in HBM (a key map); the PROBE side gets them as ordinary
 * columns (lookup columns), filled by a kernel inside the decode call.  No key and no value crosses the link.
 *
 * A KEY MAP IS A KEY SET THAT ALSO HOLDS VALUES: per distinct non-NULL key of the build side's kept rows one row of
 * 1 .. ORCGPU_KEY_MAP_MAX_VALUES value columns.  Everything said of a key set above holds for a map: the key kinds (Byte / Short /
 * Int / Long / Date, as int64), the kept rows (behind the row selection and the row filter), max_keys and its refusal at the seal,
 * rows_seen, has_null, several readers collecting into one map, the key whose value is the build's free-slot sentinel,
 * ORCGPU_KEY_SET_HASH_BITS and ORCGPU_POISON.
 *   - A SEALED MAP MAY BE NAMED BY ORCGPU_PRED_IN_SET exactly as a set is (i = orcgpu_key_map_id): an inner join is the lookup plus
 *     that leaf; one table serves both.
 *   - KEYS MUST BE UNIQUE.  A second kept row with a key already in the map -- in the same stripe, another stripe or another reader
 *     -- sets a sticky flag; orcgpu_key_map_seal then fails with ORCGPU_UNSUPPORTED, the message says "duplicate key", and the map
 *     is unusable (collect, lookup columns and predicates refuse it; free it).  Which of the two rows came first may depend on the
 *     run; whether the flag is set may not: it is set exactly when some insert found its own key already present -- for the
 *     sentinel's value, when the atomic OR of its flag returned "already set".  A NULL build key holds no values and never matches.
 *   - VALUE COLUMNS.  Byte .. Long and Date become Int64 (a Date is int64 days, as in the row filter's expressions and the computed
 *     columns); Decimal(p, s) becomes Decimal128(p, s) with the column's own precision and scale; Float / Double become Float64.  A
 *     NULL value is stored as NULL.  ORCGPU_UNSUPPORTED, the message naming the column: Boolean, String / Varchar / Char / Binary,
 *     Timestamp, a column read as a dictionary column, a nested column.  ORCGPU_INVALID_ARGUMENT: an unknown or unprojected column,
 *     a value name listed twice, zero values or more than 8.  A later collect into the same open map whose value count, kinds,
 *     precision or scale differ from the first collect's is ORCGPU_MISMATCHED_SCHEMA.
 *   - THE BUILD SIDE NAMES COLUMNS AS EVERY STAGE DOES: the key and the value columns may be computed columns or lookup columns of
 *     the BUILD reader -- they are ordinary columns by then.  So a snowflake chain is written: customer -> nation is looked up
 *     while orders -> customer is built.
 *   - orcgpu_reader_collect_map drains the reader as orcgpu_reader_collect_keys does (no batch, no copy back, no host wait per
 *     stripe); orcgpu_result_collect_map is the same for one hand-decoded result.  orcgpu_key_map_seal is the build's ONE host wait;
 *     info: the set's n_keys / has_null / rows_seen, n_values and per value its kind (ORCGPU_KEY_MAP_*), precision and scale.
 *     Sealing again returns the same info.  orcgpu_key_map_free: the handle goes now, the memory when the last reader or plan that
 *     probes it is gone -- freeing the handle under a live reader is safe.
 *   - MEMORY: the set's table (the power of two >= 2 x max_keys slots of 8 bytes, occupancy, 256 control bytes) and, allocated by
 *     the first collect, per value a plane of (slots + 1) x 8 or 16 bytes and (slots + 1) validity bytes.
 *
 * LOOKUP COLUMNS on the probe side: 1 .. ORCGPU_LOOKUP_MAX per reader, each {name, probe key column, map, value index}, over at
 * most 4 distinct (map, key column) pairs.
 *   - A row's lookup value is the map's value for the row's key.  It is NULL where the key is NULL, where the map has no such key,
 *     and where the stored value is NULL: LEFT JOIN.
 *   - The probe key is a projected flat root column of the key kinds above (anything else: ORCGPU_UNSUPPORTED by name; unknown or
 *     unprojected: ORCGPU_INVALID_ARGUMENT).  A computed or lookup column as probe key is ORCGPU_UNSUPPORTED.
 *   - Names obey the computed columns' rules (non-empty, distinct, no root column name of the file) and differ from the computed
 *     columns' names: ORCGPU_INVALID_ARGUMENT, naming it.
 *   - PLACE: lookup columns follow the file's projected columns and PRECEDE the computed ones, as nullable fields of type Int64,
 *     Decimal128(p, s) or Float64 -- in the schema and in every batch, host and device output alike, and among the names the row
 *     filter, aggregate arguments and conditions, GROUP BY keys (Int64, Decimal; Float64 stays refused), top-k keys,
 *     orcgpu_reader_collect_keys and orcgpu_reader_collect_map resolve against.
 *   - As a pruning predicate a leaf on a lookup column keeps every row group.
 *   - A computed column whose expression names a lookup column is ORCGPU_UNSUPPORTED in this version; the message says so.
 *   - ORCGPU_INVALID_ARGUMENT: an unsealed or failed map, one of another context, a value index past the map's values, a fifth pair,
 *     setting them after the reader has been built.  ORCGPU_UNSUPPORTED: a nested column in the projection.  Refusals that need the
 *     file's columns arrive with the first batch (or the aggregate / collect call), as the computed columns' do.
 * The columns are filled inside the decode call by one launch per (map, key column) pair -- ONE probe per row serves all of the
 * pair's values --, behind the last kernel that writes a column and in front of the computed columns' kernel and the call's closing
 * copy, which brings their per-batch null counts back: no host wait is added.  Such a decode call runs on one column lane.  A
 * reader without lookup columns launches, allocates and exports exactly what it did before.
 * orcgpu_result_lookup_columns does the same on a hand-decoded result, before any orcgpu_result_select / _filter /
 * _compute_columns on it: column_names names the result's columns, the lookup columns are appended behind them -- every later
 * result call then takes n more column names.  One host wait of its own.  A result whose decode failed is left alone. */
#define ORCGPU_KEY_MAP_MAX_VALUES 8
#define ORCGPU_LOOKUP_MAX 8
enum { ORCGPU_KEY_MAP_INT64 = 0, ORCGPU_KEY_MAP_DECIMAL128 = 1, ORCGPU_KEY_MAP_FLOAT64 = 2 };
typedef struct orcgpu_key_map orcgpu_key_map;
typedef struct {
  uint64_t n_keys;    /* distinct non-NULL keys                                        */
  uint64_t rows_seen; /* input rows of the collects                                    */
  int32_t has_null;   /* a kept row's key was NULL                                     */
  uint32_t n_values;  /* value columns (0: nothing was collected)                      */
  uint32_t kind[ORCGPU_KEY_MAP_MAX_VALUES];      /* ORCGPU_KEY_MAP_*                   */
  uint32_t precision[ORCGPU_KEY_MAP_MAX_VALUES]; /* Decimal128                         */
  uint32_t scale[ORCGPU_KEY_MAP_MAX_VALUES];
} orcgpu_key_map_info;
typedef struct {
  const char* name;            /* the lookup column                                    */
  const char* key_column;      /* the probe key: a projected flat root column          */
  const orcgpu_key_map* map;   /* sealed, of the reader's context                      */
  uint32_t value;              /* which of the map's value columns                     */
  uint32_t pad;
} orcgpu_lookup_spec;
int orcgpu_key_map_create(orcgpu_ctx* ctx, uint64_t max_keys, orcgpu_key_map** map);
int orcgpu_reader_collect_map(orcgpu_reader* r, const char* key_column, const char* const* value_columns, uint32_t n_values, orcgpu_key_map* map);
int orcgpu_result_collect_map(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                              const char* const* column_names, uint32_t n_columns, const char* key_column, const char* const* value_columns,
                              uint32_t n_values, orcgpu_key_map* map);
int orcgpu_key_map_seal(orcgpu_key_map* map, orcgpu_key_map_info* info);
uint64_t orcgpu_key_map_id(const orcgpu_key_map* map);
void orcgpu_key_map_free(orcgpu_key_map* map);
int orcgpu_reader_set_lookup_columns(orcgpu_reader* r, const orcgpu_lookup_spec* specs, uint32_t n);
int orcgpu_result_lookup_columns(orcgpu_ctx* ctx, orcgpu_result* result, const orcgpu_lookup_spec* specs, uint32_t n, const char* const* column_names);

/* ---- device-resident batches (Arrow C Device Data Interface, DLPack) --------------------------------------------------------------
 * A decoded result lives in HBM; the entry points above copy it to pinned host memory before a consumer sees a byte.  These
 * hand the device buffers out instead, for consumers on the same GPU (a torch model, this library's own writer with
 * ORCGPU_ENC_ON_DEVICE): nothing crosses the link.  Flat schemas only: every root column a primitive, string, binary, decimal
 * or timestamp column; a Struct, List, Map or Union column among them is ORCGPU_UNSUPPORTED, the message naming the column.
 *
 * export_batch_device: the device twin of orcgpu_result_export_batch -- the same struct array, formats, null counts and the same
 * rule of no validity buffer when the batch has no null --, every buffer pointer being the device pointer that
 * orcgpu_result_batch_view reports.  No byte is copied.  device_type is ARROW_DEVICE_ROCM, device_id the context's device, and
 * sync_event points to a hipEvent_t recorded on the decode stream behind the last work that writes the result (decode, row
 * selection, row filter): wait for it (orcgpu_device_array_wait) before reading a buffer on another stream or on the host.
 *
 * Ownership.  Every exported ArrowDeviceArray, and every DLPack tensor made from one, holds a reference on the result it views.
 * A result with references outstanding is neither decoded into again nor freed: orcgpu_result_free and orcgpu_reader_close
 * only give up the owner's claim, and the memory goes when the last reference is released (a reader that is still open then takes
 * the result back and decodes a later stripe into it; meanwhile it allocates fresh ones).  So exported batches stay valid after
 * orcgpu_result_free and orcgpu_reader_close -- but NOT after orcgpu_close: the context must outlive every exported batch and
 * tensor.  Release an array exactly once through array.release; it may be released in any thread, and with work that reads its
 * buffers still in flight on any stream of the device: before the library writes into a result that has been exported again --
 * the reader recycling it, a caller passing it to orcgpu_decode_staged once more -- it waits for the device (freeing waits, too).
 * While exports view it, a result is refused by orcgpu_decode_staged, orcgpu_result_select and orcgpu_result_filter
 * (ORCGPU_INVALID_ARGUMENT). */
int orcgpu_result_export_batch_device(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t batch, struct ArrowDeviceArray* out_array,
                                      struct ArrowSchema* out_schema);
/* A builder setter (before the first batch): on != 0 makes the reader hand out device batches through
 * orcgpu_reader_next_batch_device; it then never starts a device-to-host copy of a column buffer.  Everything else -- batch
 * size, projection, schema, byte range, shard, timestamp precision, row selection, predicate, row filter, read-ahead -- works as
 * on the host path and yields the same batches.  orcgpu_reader_next_batch on such a reader, and orcgpu_reader_next_batch_device
 * on a host reader, return ORCGPU_INVALID_ARGUMENT and leave the reader usable for the right call.  A nested column in the
 * projection fails the first batch with ORCGPU_UNSUPPORTED. */
int orcgpu_reader_set_device_output(orcgpu_reader* r, int on);
int orcgpu_reader_next_batch_device(orcgpu_reader* r, struct ArrowDeviceArray* out_array, struct ArrowSchema* out_schema);
/* Column-buffer bytes the reader has copied to the host so far (what orcgpu_result_fetch_async moves; the decoder's small
 * summaries are not counted).  0 on a device-output reader. */
int orcgpu_reader_d2h_bytes(const orcgpu_reader* r, uint64_t* bytes);
/* Bytes of the result's column buffers in HBM, as the decode (and the selection or filter after it) laid them out: what a copy back
 * of the result moves -- whole arenas, alignment gaps included; a filtered result: the kept rows' arena alone. */
uint64_t orcgpu_result_buffer_bytes(const orcgpu_result* r);
/* 1 while the reader's read-ahead threads are at work on its context (from the first batch of a reader with prefetch > 0 until its
 * last stripe is decoded, an error or orcgpu_reader_close), else 0: the context takes no other call meanwhile. */
int orcgpu_reader_reads_ahead(orcgpu_reader* r);
/* Makes `hip_stream` (a hipStream_t) wait for the array's sync_event; with a NULL stream -- which is also what HIP's default
 * stream is -- the calling thread waits instead.  An array without an event: nothing to wait for. */
int orcgpu_device_array_wait(const struct ArrowDeviceArray* array, void* hip_stream);
/* One buffer of one column of an array exported by this library as a DLPack tensor (include/orcgpu_dlpack.h: a DLManagedTensor*,
 * kDLROCM, the array's device): buffer 0 the validity bitmap (uint8, ceil(n / 8)), 1 the values (fixed width: the natural type,
 * [n]; Decimal128: int64 [n, 2], low word first; Boolean: the bitmap as uint8) or, for strings and binaries, the int32 offsets
 * [n + 1], 2 the string bytes (uint8).  A buffer the column does not have (no validity: the batch has no null), or an empty one:
 * ORCGPU_INVALID_ARGUMENT.  A dictionary-output column (ORCGPU_ARROW_DICTIONARY_UTF8): 1 the int32 keys [n], 3 the dictionary's
 * int32 offsets [entries + 1], 4 its bytes (uint8).  The tensor holds a reference of its own (see Ownership): it outlives the array;
 * its deleter drops it. */
int orcgpu_device_array_dlpack(const struct ArrowDeviceArray* array, uint32_t column, int buffer, void** out_managed_tensor);
/* Unpacks an LSB-first bitmap of n bits in device memory, from bit 0 on, to one byte per bit (0 or 1) in device memory of the
 * context's device, by a kernel on `hip_stream` (a hipStream_t; NULL is HIP's default stream).  The call does not wait.  Reads
 * ceil(n / 8) bytes, writes n bytes; neither pointer needs any alignment.  The caller orders the stream behind the bitmap's
 * producer (orcgpu_device_array_wait). */
int orcgpu_unpack_bits(orcgpu_ctx* ctx, const void* d_bits, uint64_t n, uint8_t* d_bytes, void* hip_stream);

/* ---- GPU encode: the reference's value encoders, byte for byte ------------------------------ */
/* Replace RleV2Encoder<N, S>::{write_slice, take_inner} (src/encoding/integer/rle_v2/mod.rs:255-531), ByteRleEncoder
 * (src/encoding/byte.rs:38-197) and BooleanEncoder (src/encoding/boolean.rs:119-170); the seam is PrimitiveValueEncoder
 * (src/encoding/mod.rs:36-50); a column's encoders are fed by src/writer/column.rs and flushed per stripe by
 * src/writer/stripe.rs:109-165.  The bytes are the reference encoder's own: the same runs (its greedy state machine's cuts, found
 * in parallel: device/rle_encode.hip), the same sub-encoding per run (SHORT_REPEAT / DIRECT / PATCHED_BASE / DELTA by
 * determine_variable_run_encoding's rules), the same bit widths.  tests/test_gpu_encode.py compares them with the restated
 * reference encoder (oracle/oo_encode.c).  (On two inputs the reference panics -- oo_encode.c's header --: such runs are DIRECT.)
 *
 * values / out: host memory, or device memory with ORCGPU_ENC_ON_DEVICE in flags (then nothing crosses PCIe but the size).
 * out = NULL only reports the size in *out_len; out_cap too small: ORCGPU_INVALID_ARGUMENT with the size in *out_len.
 * One call = one stream of a stripe (fewer than 2^32 - 1024 values).  Scratch memory is kept in the context between calls. */
#define ORCGPU_ENC_ON_DEVICE 1u
/* n values of int_bytes (2 / 4 / 8: the reference's N = i16 / i32 / i64) each; is_signed: SignedEncoding (zigzag), else UnsignedEncoding */
int orcgpu_encode_rle2(orcgpu_ctx* ctx, const void* values, uint64_t n, int int_bytes, int is_signed, uint32_t flags, uint8_t* out, uint64_t out_cap,
                       uint64_t* out_len);
/* = orcgpu_encode_rle2(ctx, values, n, 8, is_signed, 0, ...) */
int orcgpu_encode_rle2_i64(orcgpu_ctx* ctx, const int64_t* values, uint64_t n, int is_signed, uint8_t* out, uint64_t out_cap, uint64_t* out_len);
/* ByteRleEncoder over n bytes (Int8 columns) */
int orcgpu_encode_byte_rle(orcgpu_ctx* ctx, const void* values, uint64_t n, uint32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* out_len);
/* BooleanEncoder over an Arrow bitmap of n_bits bits (least significant bit first): PRESENT streams, Boolean DATA */
int orcgpu_encode_boolean(orcgpu_ctx* ctx, const void* bits, uint64_t n_bits, uint32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* out_len);

/* ColumnStripeEncoder::{encode_array, finish} for one Arrow array = one column of a stripe (src/writer/column.rs:103-165 primitive,
 * :196-258 Boolean, :304-391 strings / binaries; the types of src/writer/stripe.rs:175-185): only the valid rows' values reach the
 * encoders, a PRESENT stream is written when the array has a validity bitmap (array.nulls() is Some, whatever it holds).  The
 * streams come back in the order finish() returns them -- DATA, [LENGTH,] [PRESENT] -- in device memory of the context (valid until
 * its next encode call; orcgpu_encode_fetch copies one to the host). */
typedef struct orcgpu_enc_column {
  int32_t arrow_type;      /* ORCGPU_ARROW_BOOLEAN, _INT8 .. _INT64, _FLOAT32, _FLOAT64, _UTF8, _BINARY, _LARGE_UTF8, _LARGE_BINARY */
  uint32_t flags;          /* ORCGPU_ENC_ON_DEVICE: the three buffers are device memory */
  uint64_t n_rows;
  const uint8_t* validity; /* the validity bitmap, or NULL */
  const void* values;      /* fixed-width values; Boolean: the value bitmap; strings: value_data */
  const void* offsets;     /* strings: n_rows + 1 offsets, i32 (i64 for the LARGE_ types) */
} orcgpu_enc_column;
typedef struct orcgpu_enc_stream {
  int32_t kind;            /* ORC stream kind: 0 PRESENT, 1 DATA, 2 LENGTH */
  uint32_t pad;
  const uint8_t* data;     /* device memory */
  uint64_t len;
} orcgpu_enc_stream;
int orcgpu_encode_column(orcgpu_ctx* ctx, const orcgpu_enc_column* col, orcgpu_enc_stream streams[3], uint32_t* n_streams);
int orcgpu_encode_fetch(orcgpu_ctx* ctx, const orcgpu_enc_stream* stream, uint8_t* out);

/* ---- ArrowWriterBuilder / ArrowWriter (src/arrow_writer.rs:34-156) ----------------------------------------------------------
 * Arrow record batches -> an ORC file, byte for byte the reference writer's: a flat schema of Boolean, Int8..Int64, Float32/64,
 * Utf8, LargeUtf8, Binary, LargeBinary fields (a root Struct, column 0), and beyond the reference Timestamp(s/ms/us/ns, with a zone:
 * TIMESTAMP_INSTANT) and Decimal128(p, s) with 1 <= p <= 38, 0 <= s <= p (DATA, SECONDARY, [PRESENT]; every stripe footer of a file
 * with a Timestamp column carries writer_timezone "UTC").  A timestamp within the second before 1970-01-01 00:00:00 (but not on
 * it), or whose second is further from 2015 than i64 holds, has no ORC encoding: write returns ORCGPU_INVALID_ARGUMENT, nothing of
 * the batch is taken and the writer stays usable.  No index or statistics unless
 * orcgpu_writer_set_row_index asks for them (below).  Every stream is encoded on the
 * device (the encoders above); a stripe is cut where the reference's would be (after a slice of batch_size rows whose summed
 * encoder estimate exceeds stripe_byte_size) and reaches the host in one copy.  Uncompressed by default (the reference writes
 * CompressionKind::None only); orcgpu_writer_set_compression selects Snappy or LZ4, compressed on the device (below).
 * schema: an Arrow struct ("+s") of the fields.  Another type than those: ORCGPU_UNSUPPORTED at open (the reference panics).
 * Nested fields, to any depth: Struct (STRUCT: [PRESENT], DIRECT), List / LargeList (LIST: LENGTH, [PRESENT], DIRECT_V2) and
 * Map (MAP: the same; its key and value are its two children, the Arrow entries struct gets no column) over those leaves; the
 * columns are numbered in preorder and their streams written in that order.  A child column holds one entry per existing
 * row of its parent, flattened on the device from the arrays' validity, offsets and slicing.  Offsets that descend or address
 * rows beyond the child: write returns ORCGPU_INVALID_ARGUMENT, nothing of the batch is taken and the writer stays usable.
 * The stripe cut counts every column of the tree after each slice of batch_size root rows.  Still ORCGPU_UNSUPPORTED at open,
 * the message naming the field's path: FixedSizeList, ListView, Union, dictionary and run-end encoded types, and Decimal128
 * below a List or Map.  With a nested schema orcgpu_writer_set_row_index (stride > 0) and ORCGPU_ENC_ON_DEVICE batches return
 * ORCGPU_UNSUPPORTED.
 * write: the batch as an Arrow struct array with the schema it was exported with; a schema that differs from the writer's (names,
 * types, nullability, metadata): ORCGPU_UNEXPECTED.  ORCGPU_ENC_ON_DEVICE: the buffers are device memory of ctx's device (the
 * GPU reader's batches, orcgpu_result_batch_view).  What the writer needs is copied before it returns.
 * close: the open stripe (if it holds rows) and the tail; any call on the writer but take_bytes / stats / free after it:
 * ORCGPU_INVALID_ARGUMENT.  take_bytes (memory sink): out = NULL reports how many bytes wait; then drains them. */
typedef struct orcgpu_writer orcgpu_writer;
typedef struct orcgpu_writer_opts {
  uint32_t batch_size;        /* 0: 1024 */
  uint32_t pad;
  uint64_t stripe_byte_size;  /* 0: 64 MiB */
} orcgpu_writer_opts;
typedef struct orcgpu_writer_counts {
  uint64_t stripes, rows;     /* written so far */
  uint64_t bytes;             /* of the file so far */
  uint64_t round_trips;       /* host waits for the device of the writer so far: synchronisations, and the growth of its device
                                 buffers (a free waits for the device) */
  uint64_t stripe_round_trips;/* ... of them, those of the stripes' encoding and copy (two a stripe once the buffers have grown) */
  uint64_t nested_slices;     /* columns below a Struct / List / Map, summed over the writes: taken as one slice of their array ... */
  uint64_t nested_gathers;    /* ... or, rows of a null parent lying in between, gathered through a row map */
} orcgpu_writer_counts;
int orcgpu_writer_open_file(orcgpu_ctx* ctx, const char* path, const struct ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer** out);
int orcgpu_writer_open_bytes(orcgpu_ctx* ctx, const struct ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer** out);
int orcgpu_writer_write(orcgpu_writer* w, const struct ArrowSchema* schema, const struct ArrowArray* batch, uint32_t flags);
int orcgpu_writer_flush_stripe(orcgpu_writer* w);
int orcgpu_writer_close(orcgpu_writer* w);
int orcgpu_writer_take_bytes(orcgpu_writer* w, uint8_t* out, uint64_t cap, uint64_t* len);
int orcgpu_writer_stats(const orcgpu_writer* w, orcgpu_writer_counts* out);
uint64_t orcgpu_writer_stripe_rows(const orcgpu_writer* w, uint64_t stripe);  /* rows of a written stripe (0 past the last) */
void orcgpu_writer_free(orcgpu_writer* w);

/* ---- Stream compression on the device: Snappy and LZ4 (the inverse of src/compression.rs:113-195) -----------------------------
 * A stream is cut into chunks of at most block_size bytes (0: 262144, compression.rs:31; at most 2^23 - 1, the chunk header's
 * limit: ORCGPU_INVALID_ARGUMENT above it).  A chunk is a 3-byte little-endian header, len * 2 + is_original, and a raw Snappy
 * block or a raw LZ4 block (no frame) -- or the chunk's own bytes (an ORIGINAL chunk) when compressing did not make it smaller.
 * The output is the same for the same input on every run.
 *
 * set_compression: ORCGPU_COMP_NONE (the default), ORCGPU_COMP_SNAPPY or ORCGPU_COMP_LZ4; ZLIB, LZO and ZSTD:
 * ORCGPU_UNSUPPORTED.  Legal only before the first write, flush_stripe or close (ORCGPU_INVALID_ARGUMENT after).  A compressed
 * file has the stripes, rows and (decompressed) streams of the uncompressed one; its stripe footers and file footer are written
 * as original chunks.
 * compress_stream: one stream, in and out host memory, or device memory with ORCGPU_ENC_ON_DEVICE.  out = NULL reports a bound
 * in *out_len (n + 3 per chunk); out_cap must hold it. */
int orcgpu_writer_set_compression(orcgpu_writer* w, int kind, uint64_t block_size);
int orcgpu_compress_stream(orcgpu_ctx* ctx, int kind, uint64_t block_size, const void* in, uint64_t n, uint32_t flags, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_len);

/* ---- Row index and statistics of the writer ---------------------------------------------------------------------------------
 * set_row_index: ROW_INDEX streams and statistics (the reference writes neither).  stride 0 = none (the default: the file is
 * what it was without the call), else 1 .. 2^31 - 1 rows per row group (ORCGPU_INVALID_ARGUMENT otherwise); legal only before
 * the first write, flush_stripe or close, like set_compression.  Each stripe is cut into groups of `stride` rows from its first
 * row; every column, the root struct (0) included, gets a ROW_INDEX stream ahead of its data streams, with a RowIndexEntry per
 * group: the positions orcgpu_index_entry reads (PRESENT, DATA, LENGTH) and the group's ColumnStatistics.  The stripes'
 * statistics go in the Metadata section, the file's in Footer.statistics, and Footer.row_index_stride is set.  Compressed
 * files write the index and Metadata as original chunks.  Statistics: number_of_values (valid values; the root: rows), has_null,
 * and for integers min / max / sum (the sum left out when the exact sum lies outside i64), for floats min / max / sum as f64
 * (none at all when a value is NaN), for Utf8 min / max by bytes (over 1024 bytes: lower_bound / upper_bound) and the bytes,
 * for binaries the bytes, for Booleans the true count.  The stripes, rows and data streams are those of the same writes without
 * an index (index bytes do not count toward the stripe cut), and a stripe still costs two host waits. */
int orcgpu_writer_set_row_index(orcgpu_writer* w, uint64_t stride);

/* ---- String dictionaries of the writer ---------------------------------------------------------------------------------------
 * set_dictionary: key_size_threshold 0.0 = none (the default: every file, stream and count is what it is without the call); a
 * value in (0, 1] turns dictionaries on; NaN, a negative value or one above 1: ORCGPU_INVALID_ARGUMENT.  Legal only before the
 * first write, flush_stripe or close, like set_compression.
 * The rule, per stripe and per Utf8 / LargeUtf8 column (ORC STRING) at any depth of the column tree, each on its own: with n the
 * column's non-null ORC rows in the stripe and d the distinct byte strings among them, the column is written DICTIONARY_V2 in
 * that stripe iff n > 0 and (double)d <= key_size_threshold * (double)n (Apache ORC C++'s key ratio); else its streams and
 * encoding are the direct ones, byte for byte.  Binary / LargeBinary columns stay DIRECT_V2: ORC has no dictionary for BINARY.
 * A dictionary column's streams, in this order: DATA (kind 1) the n rows' ids, unsigned RLE v2 through the encoder and integer
 * width of the direct LENGTH stream; LENGTH (2) the d entries' lengths, likewise; DICTIONARY_DATA (3) the entries' bytes back to
 * back; PRESENT (0) under the unchanged rule.  ColumnEncoding: {DICTIONARY_V2, dictionary_size d}.  Entry k is the k-th distinct
 * value in the stripe's row order (the dictionary is not sorted); ids start at 0 in every stripe.  The dictionary is built on
 * the device at the flush: the file does not depend on how the device schedules the work.  The stripe cut stays the one over the
 * direct encoders' estimates, so the file has the stripes and rows of the same writes without a threshold; statistics are
 * unchanged; a row index entry of a dictionary column holds [PRESENT's positions,] then DATA's run-length positions, nothing
 * for LENGTH or DICTIONARY_DATA.  A stripe with such columns costs one host wait more, whatever their number.
 * dictionary_counts: the (string column, stripe) pairs written DICTIONARY_V2 and written DIRECT_V2 so far.
 * ORCGPU_DICT_HASH_BITS=N (1 .. 32, read when a writer is opened) keeps N bits of the strings' hash, for tests of long probe
 * sequences on small inputs; no byte of the output depends on it. */
int orcgpu_writer_set_dictionary(orcgpu_writer* w, double key_size_threshold);
int orcgpu_writer_dictionary_counts(const orcgpu_writer* w, uint64_t* dictionary, uint64_t* direct);

/* ---- Bloom filters of the writer ---------------------------------------------------------------------------------------------
 * set_bloom_filter: a BLOOM_FILTER_UTF8 stream (kind 8) for each of the n_columns named top-level fields, directly behind the
 * column's ROW_INDEX in the stripe's index region: a BloomFilterIndex with one BloomFilter {numHashFunctions, utf8bitset} per row
 * group, bit for bit what Apache ORC's writer builds, so that an equality predicate prunes row groups min / max cannot.
 * n_columns 0 = none (the default: the file is what it is without the call).  Legal only before the first write, flush_stripe
 * or close, and only after orcgpu_writer_set_row_index with a stride above 0 (which cannot be changed afterwards); fpp, the false
 * positive probability, strictly between 0 and 1; an unknown name or one listed twice: ORCGPU_INVALID_ARGUMENT otherwise.  A
 * Boolean, Timestamp or Decimal128 column: ORCGPU_UNSUPPORTED, the message naming it (INTEGRATION.md 8 says why).  A call
 * replaces the list of an earlier one; a call that fails changes nothing.
 * Size, with n the stride: numBits = (int64)(-n ln fpp / (ln 2)^2), the bitset numBits / 64 + 1 words of 64 bits, k =
 * max(1, round(numBits / n * ln 2)) hash functions (10000, 0.01: 1498 words, k = 7); a bitset above 2^30 bytes:
 * ORCGPU_INVALID_ARGUMENT.  Every row group of a listed column has a filter of that size, the short last one and one without
 * a value (all zero) too.  Nulls are not hashed.  Byte .. Long: the value as i64 through Thomas Wang's hash; Float, Double: the
 * value as a double, its bits (every NaN as 0x7ff8000000000000) through the same hash; Utf8, LargeUtf8, Binary, LargeBinary: ORC's
 * Murmur3 hash64 (seed 104729) of the bytes, whatever encoding the stripe writes the column with.  The filters are built on the
 * device at the flush; the bytes do not depend on how the device schedules the work.  Compressed files write the stream as
 * original chunks, like the row index.  Nothing else of the file changes, and a stripe costs no host wait more. */
int orcgpu_writer_set_bloom_filter(orcgpu_writer* w, const char* const* columns, uint32_t n_columns, double fpp);

/* ---- timing hooks used by bench.py (HIP events on the context's own stream) ---------------------- */
/* Milliseconds the device spent in the last orcgpu_decode_staged call, whole call and the RLE
 * expansion kernels alone (the dominant kernel), measured with hipEvents on the ctx stream. */
int orcgpu_last_timing(const orcgpu_ctx* ctx, float* total_ms, float* expand_ms, uint32_t* expand_launches);
/* The same call split into the phases of the pipeline (HIP events between them, same stream):
 *   0 block decompression (compression.rs:142-195): the block decoders' kernels
 *   1 the chunks' plain bytes strung together (Decompressor::read across chunks), run-boundary walk + output position scans
 *   2 PRESENT streams -> validity / ranks               3 RLE expansion (the three *_expand kernels)
 *   4 finishers (null spacing, strings, decimals, timestamps) + the summary copy
 *   5 (part of 0) the first stage of the block decompressors alone: Zstandard entropy decoding / Snappy and LZ4 token parsing;
 *     0 minus 5 = the LZ77 execution kernels (and DEFLATE, which is one kernel)
 *   6 (part of 5) Zstandard at table scale, where the sequences are decoded one lane per block: what runs in front of that
 *     kernel (the FSE table construction); 5 minus 6 = the sequences kernel (the literals kernel runs beside it).  0 otherwise
 * ms[0..n) receives the first n of them. */
#define ORCGPU_N_PHASES 7
int orcgpu_last_phase_ms(const orcgpu_ctx* ctx, float* ms, uint32_t n);

/* A decode call may run its columns as up to four COLUMN LANES side by side (each lane: a HIP stream of its own with the whole
 * pipeline over its share of the columns; the planner decides, ORCGPU_LANES = 1..4 forces a count -- read at every call).
 * Every lane launches its own kernels over its own bytes: a kernel's roofline figure must be priced launch by launch, with the
 * bytes THAT launch works for.  orcgpu_last_lane_stats reports lane `lane` of the last orcgpu_decode_staged call on `ctx`:
 *   n_lanes        lanes that call ran (the same in every lane's record)
 *   stream_bytes   staged (compressed) stream bytes of the columns the lane decoded      } SURVEY 8(d)'s algorithmic bytes
 *   arrow_bytes    Arrow bytes it left in the results                                     } of the lane's launches
 *   start_ms       host milliseconds from the call's entry to the lane's first launch (planning, sorting, table set-up)
 *   total_ms       first launch to the end of the lane's last kernel (HIP events on the lane's stream)
 *   phase_ms[]     the phases of orcgpu_last_phase_ms, for this lane
 *   seq_kernel_ms  Zstandard at table scale: zstd_seq_quads_kernel alone (an event in front of it and one behind it, in front of
 *                  the wait for the literals kernel that runs beside it); 0 when the call had no such launch
 *   exec_kernel_ms the LZ77 execution kernel(s) of the lane (lz_exec_wave_kernel / lz_exec_kernel / lz_exec_tokens_kernel)
 *   walk_short_kernel_ms, dict_emit_kernel_ms   rle_walk_short_kernel / dict_emit_kernel alone (events around the launch; 0: none)
 *   literals_kernel_ms   Zstandard at table scale: zstd_literals_kernel alone, on the stream it runs on beside the sequences kernel
 *                  (an event in front of it, behind the wait for the FSE tables, and one behind it); 0 when the call had no such launch
 * Returns ORCGPU_INVALID_ARGUMENT for a lane the last call did not run. */
typedef struct orcgpu_lane_stats {
  uint32_t lane, n_lanes;
  uint64_t stream_bytes, arrow_bytes;
  float start_ms, total_ms;
  float phase_ms[ORCGPU_N_PHASES];
  float seq_kernel_ms, exec_kernel_ms;
  float walk_short_kernel_ms, dict_emit_kernel_ms;
  float literals_kernel_ms;
} orcgpu_lane_stats;
int orcgpu_last_lane_stats(const orcgpu_ctx* ctx, uint32_t lane, orcgpu_lane_stats* out);

/* The HOST time of lane `lane` in the last orcgpu_decode_staged call on `ctx`, in microseconds of the lane's own thread, part
 * by part in the order they run (us[0..n) receives the first n):
 *   0 lanes     the call's entry to the lane's start: results reset, columns dealt out to the lanes
 *   1 columns   the lane's columns planned (streams, jobs, result offsets)
 *   2 chunks    plan_decompress: the chunk / block tables counted, ordered and given their workspace
 *   3 layout    job layout, workspace and result buffers, the wait for the lane's previous call, the summary's host mirror
 *               (0 .. 3 together are orcgpu_lane_stats::start_ms)
 *   4 fill      the chunk / stream / block / item tables written to pinned memory
 *   5 upload    the copies of the summary and of those tables to the device enqueued
 *   6 gate      waiting for the other lanes to enqueue their Zstandard table kernels
 *   7 decomp    the decompression launches themselves (what launch_decompress took beyond 4 .. 6)
 *   8 enqueue   every launch behind them
 *   9 wait      the last launch to the end of the lane's work on the device (the final synchronise)
 *  10 summary   the summary read: errors resolved per column, null counts, what the next call needs
 * Returns ORCGPU_INVALID_ARGUMENT for a lane the last call did not run. */
#define ORCGPU_N_HOST_PARTS 11
int orcgpu_last_lane_host_us(const orcgpu_ctx* ctx, uint32_t lane, float* us, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
