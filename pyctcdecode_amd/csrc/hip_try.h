// hip_try.h -- the one error macro of the HIP translation units (host code of .hip files only).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

// For functions that return int and have `std::string* err` in scope: a failing HIP call leaves
// "<the call's text>: <HIP's message>" in *err and returns -1.
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      if (err) *err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
      return -1;                                                                         \
    }                                                                                    \
  } while (0)
