// Argument checks that the LPIPS forward (lpips.hip) and its backward (lpips_grad.hip) share; defined in lpips.hip.
// Each returns 0, or -1 with the refusal as the error text (abi_support.h).
#pragma once
#include <stdint.h>
#include "abi_support.h"

// P pairs of h x w maps: P in [1,65535], h w below 2^31
TEXGS_HIDDEN int check_lpips_head_size(int32_t P, int32_t h, int32_t w);
// the strides of a [B, Cn, h, w] view in floats: all zero (dense), or no two elements on one address and B img below 2^62
TEXGS_HIDDEN int check_conv_strides(const char* name, int64_t row, int64_t chan, int64_t img, int64_t B, int64_t Cn, int64_t h, int64_t w);
