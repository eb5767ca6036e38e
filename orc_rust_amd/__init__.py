"""orc_rust_amd -- MI355X-native ORC stripe -> Arrow decoder (drop-in for orc-rust's
src/encoding + src/array_decoder hot path).  The compute path is hand-written HIP for gfx950 in
csrc/, reached through the C ABI of include/orcgpu.h; this package is the thin Python binding
used by the tests and the benchmark."""
from . import capi  # noqa: F401
from .arrow_reader import ArrowReader, ArrowReaderBuilder  # noqa: F401
from .arrow_writer import ArrowWriter, ArrowWriterBuilder  # noqa: F401
from .device_batch import DeviceColumn, DeviceRecordBatch  # noqa: F401
from .key_set import KeySet  # noqa: F401
from .key_map import KeyMap  # noqa: F401
from .aggregate import abs_, case, coalesce, day, day_of_week, day_of_year, divide, extract, month, nullif, quarter, when, year  # noqa: F401
from .aggregate import cast, ceil, decimal_, floor, round_, trunc  # noqa: F401
from .aggregate import decimal_ as decimal  # noqa: F401  (cast(e, decimal(2)): the Decimal128(38, 2) target)

__all__ = ["capi", "ArrowReader", "ArrowReaderBuilder", "ArrowWriter", "ArrowWriterBuilder", "DeviceColumn", "DeviceRecordBatch", "KeySet", "KeyMap",
           "year", "quarter", "month", "day", "day_of_week", "day_of_year", "extract", "divide",
           "when", "case", "coalesce", "nullif", "abs_",
           "cast", "decimal", "decimal_", "round_", "floor", "ceil", "trunc"]
