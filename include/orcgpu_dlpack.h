/*
 * orcgpu_dlpack.h -- the DLPack structs (https://dmlc.github.io/dlpack/latest/c_api.html, version 0.8: public, stable ABI) that
 * orcgpu_device_array_dlpack hands out, restated so that a caller of liborcgpu.so needs no other header.
 */
#ifndef ORCGPU_DLPACK_H
#define ORCGPU_DLPACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef DLPACK_VERSION
typedef enum {
  kDLCPU = 1,
  kDLCUDA = 2,
  kDLCUDAHost = 3,
  kDLROCM = 10,
  kDLROCMHost = 11
} DLDeviceType;

typedef struct {
  DLDeviceType device_type;
  int32_t device_id;
} DLDevice;

typedef enum { kDLInt = 0U, kDLUInt = 1U, kDLFloat = 2U, kDLOpaqueHandle = 3U, kDLBfloat = 4U, kDLComplex = 5U, kDLBool = 6U } DLDataTypeCode;

typedef struct {
  uint8_t code;   /* DLDataTypeCode */
  uint8_t bits;
  uint16_t lanes;
} DLDataType;

typedef struct {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;   /* in elements; NULL: compact row-major */
  uint64_t byte_offset;
} DLTensor;

typedef struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(struct DLManagedTensor* self);
} DLManagedTensor;
#endif

#ifdef __cplusplus
}
#endif
#endif
