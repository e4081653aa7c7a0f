// Error plumbing of the C ABI, shared by every unit that defines entry points.  The definitions and the one
// thread-local error string behind texgs_last_error() are in abi.hip; nothing here is exported from libtexgs.so.
#pragma once
#include <hip/hip_runtime.h>

#define TEXGS_HIDDEN __attribute__((visibility("hidden")))

// "<where>: <HIP's error string>" becomes the error text; returns the HIP error as itself (-1 if it is 0)
TEXGS_HIDDEN int fail(const char* where, hipError_t e);
// a refusal: msg becomes the error text; returns -1
TEXGS_HIDDEN int fail_msg(const char* msg);
// a refusal with numbers in it; returns -1
TEXGS_HIDDEN int failf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// The one place where a launcher's status (LaunchStatus, common.h) becomes a return code: a HIP error is returned as
// itself, with "<where>: <its string>" as the error text; with debug a stream sync follows and its failure is reported
// the same way.
TEXGS_HIDDEN int launched(const char* where, hipError_t st, hipStream_t s, bool debug);
