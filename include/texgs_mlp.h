/*
 * texgs_mlp.h -- the fused MLP entry points of libtexgs.so (csrc/mlp.hip): a bias-free ReLU MLP of width 128, forward and backward, on
 * the f32-input matrix cores -- what a tiny-cuda-nn Network(n_in, n_out, {"otype": "FullyFusedMLP", "activation": "ReLU",
 * "output_activation": "None", "n_neurons": 128}) computes (models/modules/utils.py:18-41 of the reference builds four of them).
 * Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.
 *
 * The function.  pad16(k) = the next multiple of 16; pin = pad16(n_in), pout = pad16(n_out), L = n_hidden_layers.
 *     params  = W_1 [128, pin] | L - 1 matrices [128, 128] | W_out [pout, 128]      row-major, back to back, f32, no biases
 *               (the layout texgs.uvnet.unpack_tcnn_params documents)
 *     xp      = [x | 1 ... 1]                    n_in columns of x, pin - n_in columns of ones
 *     h_1     = relu(W_1 xp);  h_k = relu(W_k h_{k-1});  y = (W_out h_L)[:n_out]
 * Backward for an upstream dy [N, n_out]: d_params has the full flat layout and is WRITTEN, not accumulated; rows n_out .. pout - 1 of
 * dW_out are zero; columns n_in .. pin - 1 of dW_1 are each sum_n d_1[n]; dx = (W_1^T d_1)[:, :n_in]; the ReLU masks are h > 0 of the
 * backward's own recomputation.  No atomics: two calls give bit-identical results.
 */
#ifndef TEXGS_MLP_H
#define TEXGS_MLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_MLP_WIDTH 128                     /* the only supported n_neurons */
#define TEXGS_MLP_MAX_HIDDEN_LAYERS 2
#define TEXGS_MLP_FORWARD_TILE 128              /* points per workgroup of the forward kernel */
#define TEXGS_MLP_BACKWARD_TILE 64              /* points per tile of the backward kernel */
#define TEXGS_MLP_BACKWARD_MAX_WORKGROUPS 256   /* its persistent grid: a workgroup takes tiles g, g + 256, ... */

/* Supported: n_neurons == 128, n_hidden_layers in {1, 2}, 1 <= n_in <= 128, 1 <= n_out <= 128.  Anything else is refused by name. */
typedef struct TexGSMlp {
    int32_t n_in;
    int32_t n_out;
    int32_t n_hidden_layers;
    int32_t n_neurons;
} TexGSMlp;

/* Floats of `params`; 0, with the cause in texgs_last_error(), for an unsupported shape. */
size_t texgs_mlp_param_count(const TexGSMlp* mlp);

/* Bytes of `temp` (16-byte aligned) for the calls below; 0 for an unsupported shape or N < 0.  The weights are re-packed to the
 * matrix cores' operand order into it on the call's own stream: no hidden allocation, no state between calls or streams. */
size_t texgs_mlp_forward_temp_bytes(const TexGSMlp* mlp, int32_t N);
size_t texgs_mlp_backward_temp_bytes(const TexGSMlp* mlp, int32_t N);

/* y [N, n_out] from x [N, n_in]; both row-major f32, 4-byte aligned.  One pack launch and one launch of the network; no activation
 * is stored to memory.  N == 0: success without a launch. */
int texgs_mlp_forward(const TexGSMlp* mlp, const float* params, const float* x, int32_t N, float* y, void* temp, void* stream);

/* dx [N, n_in] and d_params [texgs_mlp_param_count], each optional: a NULL output skips its products.  N == 0: success without a
 * launch, d_params zeroed. */
int texgs_mlp_backward(const TexGSMlp* mlp, const float* params, const float* x, const float* dy, int32_t N, float* dx, float* d_params,
                       void* temp, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_MLP_H */
