/* device_abi_check.c -- include/orcgpu.h as a C program sees it: the layout of struct ArrowDeviceArray is the Arrow C Device Data
 * Interface's, and the DLPack structs of include/orcgpu_dlpack.h are DLPack's. */
#include <stddef.h>
#include <stdio.h>

#define ORCGPU_ARROW_STRUCTS 1 /* the Arrow structs from the header itself */
#include "../../include/orcgpu.h"
#include "../../include/orcgpu_dlpack.h"

#define CHECK(cond)                      \
  do {                                   \
    if (!(cond)) {                       \
      printf("FAILED %s\n", #cond);      \
      return 1;                          \
    }                                    \
  } while (0)

int main(void) {
  CHECK(sizeof(struct ArrowArray) == 80);
  CHECK(sizeof(struct ArrowSchema) == 72);
  CHECK(sizeof(struct ArrowDeviceArray) == 128);
  CHECK(offsetof(struct ArrowDeviceArray, array) == 0);
  CHECK(offsetof(struct ArrowDeviceArray, device_id) == 80);
  CHECK(offsetof(struct ArrowDeviceArray, device_type) == 88);
  CHECK(offsetof(struct ArrowDeviceArray, sync_event) == 96);
  CHECK(offsetof(struct ArrowDeviceArray, reserved) == 104);
  CHECK(ARROW_DEVICE_ROCM == 10);
  CHECK(ORCGPU_ABI_VERSION == 4);
  CHECK(kDLROCM == 10);
  CHECK(sizeof(DLDataType) == 4);
  CHECK(sizeof(DLTensor) == 48);
  CHECK(offsetof(DLTensor, shape) == 24);
  CHECK(offsetof(DLManagedTensor, manager_ctx) == 48);
  CHECK(offsetof(DLManagedTensor, deleter) == 56);
  printf("ok\n");
  return 0;
}
