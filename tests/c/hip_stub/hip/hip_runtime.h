// Just enough of the HIP runtime's names for gpslc_internal.h to compile as plain host C++ (tests/c/tri_decode_test.cpp): the
// qualifiers expand to nothing and the runtime calls the header's inline helpers make are declared, never called.
#pragma once
#include <cmath>
#define __host__
#define __device__
#define __forceinline__ inline
typedef struct ihipStream_t* hipStream_t;
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize };
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount };
int hipGetDevice(int*);
int hipFuncSetAttribute(const void*, hipFuncAttribute, int);
int hipDeviceGetAttribute(int*, hipDeviceAttribute_t, int);
struct { unsigned x, y, z; } static const threadIdx = {0, 0, 0};
