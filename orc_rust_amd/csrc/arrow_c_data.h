// arrow_c_data.h -- the Arrow C Data Interface structs (public, stable ABI)
#pragma once
#include <cstdint>

extern "C" {
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
// ... and the Arrow C Device Data Interface
#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  int32_t device_type;
  void* sync_event;
  int64_t reserved[3];
};
#endif
}
