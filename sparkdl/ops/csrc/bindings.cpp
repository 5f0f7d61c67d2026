// Torch extension bindings for sparkdl's CDNA4 kernels (sparkdl._C).
//
// Host-only translation layer: validates tensors, allocates outputs and
// workspaces through ATen, and launches the pure-HIP kernels declared in
// kernels.h on the current HIP stream.

#include <torch/extension.h>
// ROCm torch masquerades HIP devices as DeviceType::CUDA; the plain
// c10::hip guard/stream APIs reject such devices, so the
// MasqueradingAsCUDA variants are the native entry points.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cmath>
#include <utility>
#include <vector>

#include "kernels.h"

namespace {

using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

#define CHECK_BF16_CUDA(t)                                            \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                   \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16");\
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

#define CHECK_F32_CUDA(t)                                             \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");                   \
  TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be fp32");   \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

const short* bf_ptr(const at::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr<at::BFloat16>());
}
short* bf_ptr_mut(at::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr<at::BFloat16>());
}

// ---------------------------------------------------------------------
// Fused optimizers (multi-tensor table built Python-side as blobs)
// ---------------------------------------------------------------------

void fused_adamw_(const at::Tensor& chunks_blob, const at::Tensor& bmap,
                  int64_t nblocks, double lr, double beta1, double beta2,
                  double eps, double weight_decay, at::Tensor step_counter,
                  at::Tensor coeffs) {
  TORCH_CHECK(chunks_blob.is_cuda() && bmap.is_cuda());
  TORCH_CHECK(step_counter.is_cuda() &&
              step_counter.scalar_type() == at::kLong);
  TORCH_CHECK(coeffs.is_cuda() && coeffs.scalar_type() == at::kFloat &&
              coeffs.numel() >= 2);
  DeviceGuard guard(chunks_blob.device());
  launch_fused_adamw(
      reinterpret_cast<const TensorChunk*>(chunks_blob.data_ptr()),
      reinterpret_cast<const int2*>(bmap.data_ptr()), (int)nblocks,
      (float)lr, (float)beta1, (float)beta2, (float)eps,
      (float)weight_decay,
      reinterpret_cast<long long*>(step_counter.data_ptr<int64_t>()),
      coeffs.data_ptr<float>(), cur_stream());
}

void zero_grads_(const at::Tensor& chunks_blob, const at::Tensor& bmap,
                 int64_t nblocks) {
  TORCH_CHECK(chunks_blob.is_cuda() && bmap.is_cuda());
  DeviceGuard guard(chunks_blob.device());
  launch_zero_grads(
      reinterpret_cast<const TensorChunk*>(chunks_blob.data_ptr()),
      reinterpret_cast<const int2*>(bmap.data_ptr()), (int)nblocks,
      cur_stream());
}

void fused_sgd_(const at::Tensor& chunks_blob, const at::Tensor& bmap,
                int64_t nblocks, double lr, double momentum,
                double weight_decay, bool nesterov, bool first_step) {
  TORCH_CHECK(chunks_blob.is_cuda() && bmap.is_cuda());
  DeviceGuard guard(chunks_blob.device());
  launch_fused_sgd(
      reinterpret_cast<const TensorChunk*>(chunks_blob.data_ptr()),
      reinterpret_cast<const int2*>(bmap.data_ptr()), (int)nblocks,
      (float)lr, (float)momentum, (float)weight_decay, nesterov,
      first_step, cur_stream());
}

// ---------------------------------------------------------------------
// LayerNorm
// ---------------------------------------------------------------------

std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x,
                                      const at::Tensor& gamma,
                                      const at::Tensor& beta, double eps) {
  CHECK_BF16_CUDA(x);
  CHECK_F32_CUDA(gamma);
  CHECK_F32_CUDA(beta);
  DeviceGuard guard(x.device());
  const int cols = (int)x.size(-1);
  const int rows = (int)(x.numel() / cols);
  TORCH_CHECK(gamma.numel() == cols && beta.numel() == cols);

  auto y = at::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  auto mean = at::empty({rows}, f32);
  auto rstd = at::empty({rows}, f32);
  launch_layernorm_fwd(bf_ptr(x), gamma.data_ptr<float>(),
                       beta.data_ptr<float>(), bf_ptr_mut(y),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       rows, cols, (float)eps, cur_stream());
  return {y, mean, rstd};
}

std::vector<at::Tensor> layernorm_bwd(const at::Tensor& x,
                                      const at::Tensor& dy,
                                      const at::Tensor& gamma,
                                      const at::Tensor& mean,
                                      const at::Tensor& rstd) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(dy);
  CHECK_F32_CUDA(gamma);
  DeviceGuard guard(x.device());
  const int cols = (int)x.size(-1);
  const int rows = (int)(x.numel() / cols);
  TORCH_CHECK(cols <= 8192, "layernorm_bwd LDS partials support cols<=8192");

  auto dx = at::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  const int blocks = layernorm_bwd_part_rows(rows);
  const int ws_rows = blocks * 4;  // one partial row per wave
  auto dgamma_part = at::empty({ws_rows, cols}, f32);
  auto dbeta_part = at::empty({ws_rows, cols}, f32);
  // zero-init: the 2D reduce kernel folds row-splits with atomics
  auto dgamma = at::zeros({cols}, f32);
  auto dbeta = at::zeros({cols}, f32);
  launch_layernorm_bwd(bf_ptr(x), bf_ptr(dy), gamma.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       bf_ptr_mut(dx), dgamma_part.data_ptr<float>(),
                       dbeta_part.data_ptr<float>(), blocks, rows, cols,
                       cur_stream());
  launch_layernorm_reduce_parts(
      dgamma_part.data_ptr<float>(), dbeta_part.data_ptr<float>(),
      dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), ws_rows, cols,
      cur_stream());
  return {dx, dgamma, dbeta};
}

// ---------------------------------------------------------------------
// BatchNorm (+add) (+ReLU), NHWC bf16
// ---------------------------------------------------------------------

// Shared validation; returns {rows, cols} of x. chan: the per-channel
// tensors of the call. act: its tensors of x's shape, null where an
// optional one is absent. With relu, mask is the forward's bit mask.
static std::pair<long long, int> bn_check(
    const char* op, const at::Tensor& x,
    std::initializer_list<const at::Tensor*> chan,
    std::initializer_list<const at::Tensor*> act, bool relu = false,
    const at::Tensor* mask = nullptr) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  x.is_contiguous() && x.dim() >= 1,
              op, ": x must be a contiguous bf16 GPU tensor");
  const int64_t cols = x.size(-1);
  TORCH_CHECK(cols > 0 && cols % 8 == 0 && cols <= 2048, op,
              " requires cols%8==0 and cols<=2048 (NHWC channels), got ",
              cols);
  for (const at::Tensor* t : chan)
    TORCH_CHECK(t->is_cuda() && t->device() == x.device() &&
                    t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->numel() == cols,
                op, ": per-channel tensors must be contiguous fp32 of ",
                cols, " elements on x's device");
  for (const at::Tensor* t : act)
    TORCH_CHECK(!t || (t->is_cuda() && t->device() == x.device() &&
                       t->scalar_type() == at::kBFloat16 &&
                       t->is_contiguous() && t->sizes() == x.sizes()),
                op, ": activations and gradients must be contiguous bf16 ",
                x.sizes(), " on x's device");
  TORCH_CHECK(!relu || (mask->is_cuda() && mask->device() == x.device() &&
                        mask->scalar_type() == at::kByte &&
                        mask->is_contiguous() &&
                        mask->numel() == x.numel() / 8),
              op, ": relu backward needs the forward's activation mask, "
              "contiguous uint8 of ", x.numel() / 8,
              " elements on x's device");
  return {x.numel() / cols, (int)cols};
}

static const at::Tensor* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? &t.value() : nullptr;
}

// With relu the forward packs 1 bit per element, which backward uses
// instead of re-reading y; without, the mask is empty and not touched.
static at::Tensor bn_alloc_mask(const at::Tensor& x, bool relu) {
  return at::empty({relu ? x.numel() / 8 : 0},
                   x.options().dtype(at::kByte));
}
static unsigned char* mask_ptr(const at::Tensor& mask, bool relu) {
  return relu ? mask.data_ptr<unsigned char>() : nullptr;
}

std::vector<at::Tensor> bn_fwd(const at::Tensor& x,
                               const c10::optional<at::Tensor>& res,
                               const at::Tensor& gamma,
                               const at::Tensor& beta,
                               at::Tensor running_mean,
                               at::Tensor running_var, double momentum,
                               double eps, bool training, bool relu) {
  const auto [rows, cols] = bn_check(
      "bn_fwd", x, {&gamma, &beta, &running_mean, &running_var},
      {opt_ptr(res)});
  DeviceGuard guard(x.device());
  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto save_mean = at::empty({cols}, f32);
  auto save_rstd = at::empty({cols}, f32);
  // partial-sum slab + coefficients; fully written before it is read
  auto scratch = at::empty({bn_scratch_floats(rows, cols)}, f32);
  auto mask = bn_alloc_mask(x, relu);
  launch_bn_fwd(bf_ptr(x), res ? bf_ptr(*res) : nullptr,
                gamma.data_ptr<float>(), beta.data_ptr<float>(),
                running_mean.data_ptr<float>(),
                running_var.data_ptr<float>(), save_mean.data_ptr<float>(),
                save_rstd.data_ptr<float>(), scratch.data_ptr<float>(),
                bf_ptr_mut(y), mask_ptr(mask, relu), rows, cols,
                (float)momentum, (float)eps, training, relu, cur_stream());
  return {y, save_mean, save_rstd, mask};
}

// bn_fwd in training mode over a slab of partial sums [G, 2*cols] that
// the producer of x wrote (conv1x1_stats): no statistics pass.
std::vector<at::Tensor> bn_fwd_slab(const at::Tensor& x,
                                    const c10::optional<at::Tensor>& res,
                                    const at::Tensor& slab,
                                    const at::Tensor& gamma,
                                    const at::Tensor& beta,
                                    at::Tensor running_mean,
                                    at::Tensor running_var, double momentum,
                                    double eps, bool relu) {
  const auto [rows, cols] = bn_check(
      "bn_fwd_slab", x, {&gamma, &beta, &running_mean, &running_var},
      {opt_ptr(res)});
  CHECK_F32_CUDA(slab);
  TORCH_CHECK(slab.dim() == 2 && slab.size(0) >= 1 &&
                  slab.size(1) == 2 * (int64_t)cols &&
                  slab.device() == x.device(),
              "bn_fwd_slab: slab must be [G, 2*cols] on x's device");
  DeviceGuard guard(x.device());
  auto f32 = x.options().dtype(at::kFloat);
  auto y = at::empty_like(x);
  auto save_mean = at::empty({cols}, f32);
  auto save_rstd = at::empty({cols}, f32);
  auto coef = at::empty({2 * (int64_t)cols}, f32);
  auto mask = bn_alloc_mask(x, relu);
  launch_bn_fwd_slab(bf_ptr(x), res ? bf_ptr(*res) : nullptr,
                     slab.data_ptr<float>(), (int)slab.size(0),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     running_mean.data_ptr<float>(),
                     running_var.data_ptr<float>(),
                     save_mean.data_ptr<float>(),
                     save_rstd.data_ptr<float>(), coef.data_ptr<float>(),
                     bf_ptr_mut(y), mask_ptr(mask, relu), rows, cols,
                     (float)momentum, (float)eps, relu, cur_stream());
  return {y, save_mean, save_rstd, mask};
}

std::vector<at::Tensor> bn_bwd(const at::Tensor& x,
                               const at::Tensor& mask,
                               const at::Tensor& dy,
                               const at::Tensor& gamma,
                               const at::Tensor& save_mean,
                               const at::Tensor& save_rstd, bool training,
                               bool relu, bool needs_dres) {
  const auto [rows, cols] = bn_check(
      "bn_bwd", x, {&gamma, &save_mean, &save_rstd}, {&dy}, relu, &mask);
  DeviceGuard guard(x.device());
  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto dgamma = at::empty({cols}, f32);
  auto dbeta = at::empty({cols}, f32);
  auto scratch = at::empty({bn_scratch_floats(rows, cols)}, f32);
  at::Tensor dres;
  short* dres_ptr = nullptr;
  if (needs_dres) {
    dres = at::empty_like(x);
    dres_ptr = bf_ptr_mut(dres);
  }
  launch_bn_bwd(bf_ptr(x), mask_ptr(mask, relu), bf_ptr(dy),
                gamma.data_ptr<float>(),
                save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                scratch.data_ptr<float>(), dgamma.data_ptr<float>(),
                dbeta.data_ptr<float>(), bf_ptr_mut(dx), dres_ptr, rows,
                cols, training, relu, cur_stream());
  if (needs_dres) return {dx, dgamma, dbeta, dres};
  return {dx, dgamma, dbeta};
}

// bn_bwd for an output that had two consumers: dy = dy_a + dy_b is
// formed inside the reduce kernel. Returns dx, dgamma, dbeta and
// s = dy * mask, the gradient of the forward's residual input.
std::vector<at::Tensor> bn_bwd2(const at::Tensor& x,
                                const at::Tensor& mask,
                                const at::Tensor& dy_a,
                                const at::Tensor& dy_b,
                                const at::Tensor& gamma,
                                const at::Tensor& save_mean,
                                const at::Tensor& save_rstd, bool training,
                                bool relu) {
  const auto [rows, cols] =
      bn_check("bn_bwd2", x, {&gamma, &save_mean, &save_rstd},
               {&dy_a, &dy_b}, relu, &mask);
  DeviceGuard guard(x.device());
  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto s = at::empty_like(x);
  auto dgamma = at::empty({cols}, f32);
  auto dbeta = at::empty({cols}, f32);
  auto scratch = at::empty({bn_scratch_floats(rows, cols)}, f32);
  launch_bn_bwd2(bf_ptr(x), mask_ptr(mask, relu), bf_ptr(dy_a),
                 bf_ptr(dy_b), gamma.data_ptr<float>(),
                 save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                 scratch.data_ptr<float>(), dgamma.data_ptr<float>(),
                 dbeta.data_ptr<float>(), bf_ptr_mut(dx), bf_ptr_mut(s),
                 rows, cols, training, relu, cur_stream());
  return {dx, dgamma, dbeta, s};
}

// BatchNorm + ReLU + MaxPool2d(3, 2, 1) in one chain; x is [N,H,W,C].
std::vector<at::Tensor> bn_pool_fwd(const at::Tensor& x,
                                    const at::Tensor& gamma,
                                    const at::Tensor& beta,
                                    at::Tensor running_mean,
                                    at::Tensor running_var, double momentum,
                                    double eps, bool training) {
  const int cols = bn_check("bn_pool_fwd", x,
                            {&gamma, &beta, &running_mean, &running_var},
                            {}).second;
  TORCH_CHECK(x.dim() == 4, "bn_pool_fwd takes x as [N,H,W,C]");
  DeviceGuard guard(x.device());
  const int64_t n = x.size(0), h = x.size(1), w = x.size(2);
  TORCH_CHECK(n > 0 && h > 0 && w > 0 && n * h * w < (1LL << 31),
              "bn_pool_fwd requires 0 < N*H*W < 2^31");
  const int64_t ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  auto f32 = x.options().dtype(at::kFloat);
  auto pooled = at::empty({n, ho, wo, cols}, x.options());
  auto code = at::empty({n, ho, wo, cols}, x.options().dtype(at::kByte));
  auto save_mean = at::empty({cols}, f32);
  auto save_rstd = at::empty({cols}, f32);
  auto scratch = at::empty({bn_scratch_floats(n * h * w, cols)}, f32);
  launch_bn_pool_fwd(bf_ptr(x), gamma.data_ptr<float>(),
                     beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                     running_var.data_ptr<float>(),
                     save_mean.data_ptr<float>(),
                     save_rstd.data_ptr<float>(), scratch.data_ptr<float>(),
                     bf_ptr_mut(pooled), code.data_ptr<unsigned char>(),
                     (int)n, (int)h, (int)w, cols, (float)momentum,
                     (float)eps, training, cur_stream());
  return {pooled, save_mean, save_rstd, code};
}

std::vector<at::Tensor> bn_pool_bwd(const at::Tensor& x,
                                    const at::Tensor& code,
                                    const at::Tensor& dyp,
                                    const at::Tensor& gamma,
                                    const at::Tensor& save_mean,
                                    const at::Tensor& save_rstd,
                                    bool training) {
  const int cols = bn_check("bn_pool_bwd", x,
                            {&gamma, &save_mean, &save_rstd}, {}).second;
  CHECK_BF16_CUDA(dyp);
  TORCH_CHECK(x.dim() == 4, "bn_pool_bwd takes x as [N,H,W,C]");
  DeviceGuard guard(x.device());
  const int64_t n = x.size(0), h = x.size(1), w = x.size(2);
  TORCH_CHECK(n > 0 && h > 0 && w > 0 && n * h * w < (1LL << 31),
              "bn_pool_bwd requires 0 < N*H*W < 2^31");
  const int64_t ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const std::vector<int64_t> pshape = {n, ho, wo, (int64_t)cols};
  TORCH_CHECK(dyp.sizes() == at::IntArrayRef(pshape) &&
                  dyp.device() == x.device(),
              "pooled grad must be [N,Ho,Wo,C] on x's device");
  TORCH_CHECK(code.is_cuda() && code.device() == x.device() &&
              code.scalar_type() == at::kByte && code.is_contiguous() &&
              code.sizes() == at::IntArrayRef(pshape),
              "backward needs the forward's tap codes");
  auto f32 = x.options().dtype(at::kFloat);
  auto dx = at::empty_like(x);
  auto dgamma = at::empty({cols}, f32);
  auto dbeta = at::empty({cols}, f32);
  auto scratch = at::empty({bn_scratch_floats(n * h * w, cols)}, f32);
  launch_bn_pool_bwd(bf_ptr(x), code.data_ptr<unsigned char>(),
                     bf_ptr(dyp), gamma.data_ptr<float>(),
                     save_mean.data_ptr<float>(),
                     save_rstd.data_ptr<float>(), scratch.data_ptr<float>(),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
                     bf_ptr_mut(dx), (int)n, (int)h, (int)w, cols, training,
                     cur_stream());
  return {dx, dgamma, dbeta};
}

// ---------------------------------------------------------------------
// Bias + GELU
// ---------------------------------------------------------------------

at::Tensor bias_gelu_fwd(const at::Tensor& x, const at::Tensor& bias) {
  CHECK_BF16_CUDA(x);
  CHECK_F32_CUDA(bias);
  DeviceGuard guard(x.device());
  const int cols = (int)x.size(-1);
  const long long rows = x.numel() / cols;
  TORCH_CHECK(bias.numel() == cols);
  auto y = at::empty_like(x);
  launch_bias_gelu_fwd(bf_ptr(x), bias.data_ptr<float>(), bf_ptr_mut(y),
                       rows, cols, cur_stream());
  return y;
}

std::vector<at::Tensor> bias_gelu_bwd(const at::Tensor& x,
                                      const at::Tensor& bias,
                                      const at::Tensor& dy) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(dy);
  CHECK_F32_CUDA(bias);
  DeviceGuard guard(x.device());
  const int cols = (int)x.size(-1);
  const long long rows = x.numel() / cols;
  TORCH_CHECK(cols <= 16384, "bias_gelu_bwd LDS partials support cols<=16384");
  auto dx = at::empty_like(x);
  auto dbias = at::zeros({cols}, x.options().dtype(at::kFloat));
  launch_bias_gelu_bwd(bf_ptr(x), bias.data_ptr<float>(), bf_ptr(dy),
                       bf_ptr_mut(dx), dbias.data_ptr<float>(), rows, cols,
                       cur_stream());
  return {dx, dbias};
}

// ---------------------------------------------------------------------
// MFMA GEMM + bias(+GELU)
// ---------------------------------------------------------------------

std::vector<at::Tensor> gemm_bias_act(const at::Tensor& A,
                                      const at::Tensor& W,
                                      const c10::optional<at::Tensor>& bias,
                                      int64_t act, bool save_z) {
  CHECK_BF16_CUDA(A);
  CHECK_BF16_CUDA(W);
  TORCH_CHECK(A.dim() == 2 && W.dim() == 2 && A.size(1) == W.size(1));
  const int M = (int)A.size(0), K = (int)A.size(1), N = (int)W.size(0);
  TORCH_CHECK(gemm_bias_act_supported(M, N, K),
              "gemm_bias_act requires K % 64 == 0");
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    CHECK_F32_CUDA(bias.value());
    TORCH_CHECK(bias->numel() == N);
    bias_ptr = bias->data_ptr<float>();
  }
  DeviceGuard guard(A.device());
  auto C = at::empty({M, N}, A.options());
  at::Tensor Z;
  short* z_ptr = nullptr;
  if (save_z && act != 0) {
    Z = at::empty({M, N}, A.options());
    z_ptr = bf_ptr_mut(Z);
  }
  launch_gemm_bias_act(bf_ptr(A), bf_ptr(W), bias_ptr, bf_ptr_mut(C),
                       z_ptr, M, N, K, (int)act, cur_stream());
  if (z_ptr) return {C, Z};
  return {C};
}

// ---------------------------------------------------------------------
// Fused vocabulary projection + cross-entropy
// ---------------------------------------------------------------------

// Shared validation of h [M,K], weight [V,K], bias [V] and labels [M].
static const float* lce_check(const char* op, const at::Tensor& h,
                              const at::Tensor& weight,
                              const c10::optional<at::Tensor>& bias,
                              const at::Tensor& labels) {
  CHECK_BF16_CUDA(h);
  CHECK_BF16_CUDA(weight);
  TORCH_CHECK(h.dim() == 2 && weight.dim() == 2 &&
                  h.size(1) == weight.size(1),
              op, " takes h [M,K] and weight [V,K], got ", h.sizes(), " and ",
              weight.sizes());
  TORCH_CHECK(lce_supported(h.size(0), weight.size(0), h.size(1)), op,
              " requires K % 64 == 0, M >= 1 and 1 <= V <= 2^30, got h ",
              h.sizes(), " weight ", weight.sizes());
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                  labels.is_contiguous() && labels.dim() == 1 &&
                  labels.size(0) == h.size(0),
              op, ": labels must be contiguous int64 [M] on the GPU");
  TORCH_CHECK(weight.device() == h.device() && labels.device() == h.device(),
              op, ": tensors must share one device");
  if (!bias.has_value()) return nullptr;
  CHECK_F32_CUDA(bias.value());
  TORCH_CHECK(bias->numel() == weight.size(0) &&
                  bias->device() == h.device(),
              op, ": bias must hold V fp32 values on h's device");
  return bias->data_ptr<float>();
}

// -> {loss, lse [M], count int32 [1]}; loss is per row [M] for "none",
// a 0-dim tensor for "sum" and "mean" (the sum over max(count, 1)).
std::vector<at::Tensor> lce_forward(const at::Tensor& h,
                                    const at::Tensor& weight,
                                    const c10::optional<at::Tensor>& bias,
                                    const at::Tensor& labels,
                                    int64_t ignore_index,
                                    const std::string& reduction) {
  const float* bias_ptr = lce_check("lce_forward", h, weight, bias, labels);
  TORCH_CHECK(reduction == "none" || reduction == "sum" ||
                  reduction == "mean",
              "lce_forward: reduction must be none, sum or mean, got ",
              reduction);
  DeviceGuard guard(h.device());
  const int M = (int)h.size(0), K = (int)h.size(1), V = (int)weight.size(0);
  auto f32 = h.options().dtype(at::kFloat);
  auto ws = at::empty({(int64_t)lce_vtiles(V), M, 2}, f32);
  auto zlab = at::empty({M}, f32);
  auto loss = at::empty({M}, f32);
  auto lse = at::empty({M}, f32);
  auto count = at::empty({1}, h.options().dtype(at::kInt));
  at::Tensor total;
  if (reduction != "none") total = at::empty({}, f32);
  launch_lce_forward(bf_ptr(h), bf_ptr(weight), bias_ptr,
                     reinterpret_cast<const long long*>(
                         labels.data_ptr<int64_t>()),
                     reinterpret_cast<float2*>(ws.data_ptr<float>()),
                     zlab.data_ptr<float>(), loss.data_ptr<float>(),
                     lse.data_ptr<float>(), count.data_ptr<int>(),
                     total.defined() ? total.data_ptr<float>() : nullptr,
                     reduction == "mean", M, V, K, ignore_index,
                     cur_stream());
  return {total.defined() ? total : loss, lse, count};
}

// -> {dZ [M,V] bf16, a view of rows lce_ldz(V) elements apart whose
// padding columns are zero; dbias [V] fp32}. gout: fp32, one value or
// one per row; count (the forward's) divides it, for "mean".
std::vector<at::Tensor> lce_backward(const at::Tensor& h,
                                     const at::Tensor& weight,
                                     const c10::optional<at::Tensor>& bias,
                                     const at::Tensor& labels,
                                     const at::Tensor& lse,
                                     const at::Tensor& gout,
                                     const c10::optional<at::Tensor>& count,
                                     int64_t ignore_index) {
  const float* bias_ptr = lce_check("lce_backward", h, weight, bias, labels);
  CHECK_F32_CUDA(lse);
  CHECK_F32_CUDA(gout);
  const int M = (int)h.size(0), K = (int)h.size(1), V = (int)weight.size(0);
  TORCH_CHECK(lse.numel() == M && lse.device() == h.device(),
              "lce_backward: lse must hold M fp32 values on h's device");
  TORCH_CHECK((gout.numel() == 1 || gout.numel() == M) &&
                  gout.device() == h.device(),
              "lce_backward: gout must hold 1 or M fp32 values on h's "
              "device, got ", gout.numel());
  const int* count_ptr = nullptr;
  if (count.has_value()) {
    TORCH_CHECK(count->is_cuda() && count->device() == h.device() &&
                    count->scalar_type() == at::kInt && count->numel() == 1,
                "lce_backward: count must be int32 [1] on h's device");
    count_ptr = count->data_ptr<int>();
  }
  DeviceGuard guard(h.device());
  const int64_t ldz = lce_ldz(V);
  auto f32 = h.options().dtype(at::kFloat);
  auto dz = at::empty({M, ldz}, h.options());
  auto slab = at::empty({(int64_t)lce_bands(M), ldz}, f32);
  auto dbias = at::empty({V}, f32);
  launch_lce_backward(bf_ptr(h), bf_ptr(weight), bias_ptr,
                      reinterpret_cast<const long long*>(
                          labels.data_ptr<int64_t>()),
                      lse.data_ptr<float>(), gout.data_ptr<float>(),
                      gout.numel() == 1 ? 0 : 1, count_ptr, bf_ptr_mut(dz),
                      slab.data_ptr<float>(), dbias.data_ptr<float>(), M, V,
                      K, ignore_index, cur_stream());
  return {dz.narrow(1, 0, V), dbias};
}

at::Tensor gemm_stream(const at::Tensor& A, const at::Tensor& W) {
  CHECK_BF16_CUDA(A);
  CHECK_BF16_CUDA(W);
  TORCH_CHECK(A.dim() == 2 && W.dim() == 2 && A.size(1) == W.size(1));
  const long long M = A.size(0);
  const int K = (int)A.size(1), N = (int)W.size(0);
  TORCH_CHECK(gemm_stream_supported(M, N, K),
              "gemm_stream requires K in {64,128,256} and N % 64 == 0");
  DeviceGuard guard(A.device());
  auto C = at::empty({M, N}, A.options());
  launch_gemm_stream(bf_ptr(A), bf_ptr(W), bf_ptr_mut(C), M, N, K,
                     cur_stream());
  return C;
}

// C = A @ W^T and the BatchNorm partial sums of C, A read once.
// Returns {C [M,N] bf16, slab [G, 2N] fp32}; a slab passed in (tests)
// must have exactly that shape and is the one written and returned.
std::vector<at::Tensor> conv1x1_stats(
    const at::Tensor& A, const at::Tensor& W, int64_t max_workers,
    const c10::optional<at::Tensor>& slab_out) {
  CHECK_BF16_CUDA(A);
  CHECK_BF16_CUDA(W);
  TORCH_CHECK(A.dim() == 2 && W.dim() == 2 && A.size(1) == W.size(1));
  TORCH_CHECK(W.device() == A.device());
  const long long M = A.size(0);
  const int K = (int)A.size(1), N = (int)W.size(0);
  TORCH_CHECK(conv1x1_stats_supported(M, N, K),
              "conv1x1_stats requires K in {64,128,256}, N % 64 == 0 and "
              "M >= 1");
  TORCH_CHECK(max_workers >= 0 && max_workers < (1 << 20));
  DeviceGuard guard(A.device());
  int nch, G;
  conv1x1_stats_plan(M, N, K, (int)max_workers, &nch, &G);
  auto C = at::empty({M, N}, A.options());
  at::Tensor slab;
  if (slab_out.has_value()) {
    slab = slab_out.value();
    CHECK_F32_CUDA(slab);
    TORCH_CHECK(slab.device() == A.device() && slab.dim() == 2 &&
                    slab.size(0) == G && slab.size(1) == 2 * (int64_t)N,
                "conv1x1_stats: slab must be [", G, ", ", 2 * N, "]");
  } else {
    slab = at::empty({G, 2 * (int64_t)N}, A.options().dtype(at::kFloat));
  }
  launch_conv1x1_stats(bf_ptr(A), bf_ptr(W), bf_ptr_mut(C),
                       slab.data_ptr<float>(), M, N, K, (int)max_workers,
                       cur_stream());
  return {C, slab};
}

std::vector<int64_t> conv1x1_stats_plan_py(int64_t M, int64_t N, int64_t K,
                                           int64_t max_workers) {
  TORCH_CHECK(conv1x1_stats_supported(M, (int)N, (int)K));
  int nch, G;
  conv1x1_stats_plan(M, (int)N, (int)K, (int)max_workers, &nch, &G);
  return {nch, G};
}

// ---------------------------------------------------------------------
// 3x3 stride-1 pad-1 convolution, NHWC bf16
// ---------------------------------------------------------------------

// y [N,H,W,Cout] = conv3x3(x [N,H,W,Cin], wt [Cout,3,3,Cin]), zero
// padding, no bias. Also the data gradient, on dy and the flipped,
// channel-swapped weight.
at::Tensor conv3x3(const at::Tensor& x, const at::Tensor& wt,
                   int64_t max_workers) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wt);
  TORCH_CHECK(wt.device() == x.device(),
              "conv3x3: x and wt must share one device");
  TORCH_CHECK(x.dim() == 4 && wt.dim() == 4,
              "conv3x3 takes x as [N,H,W,Cin] and wt as [Cout,3,3,Cin]");
  TORCH_CHECK(wt.size(3) == x.size(3), "conv3x3: x has ", x.size(3),
              " input channels, wt has ", wt.size(3));
  TORCH_CHECK(wt.size(1) == 3 && wt.size(2) == 3,
              "conv3x3 takes 3x3 taps, got ", wt.size(1), "x", wt.size(2));
  const int64_t n = x.size(0), h = x.size(1), w = x.size(2);
  const int64_t cin = x.size(3), cout = wt.size(0);
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
                  conv3x3_supported(n, h, w, (int)cin, (int)cout),
              "conv3x3 requires Cin and Cout multiples of 64, 1 <= W <= 56,"
              " H >= 1 and N*H*W < 2^31, got x ", x.sizes(), " wt ",
              wt.sizes());
  TORCH_CHECK(max_workers >= 0 && max_workers < (1 << 20));
  DeviceGuard guard(x.device());
  auto y = at::empty({n, h, w, cout}, x.options());
  launch_conv3x3(bf_ptr(x), bf_ptr(wt), bf_ptr_mut(y), (int)n, (int)h,
                 (int)w, (int)cin, (int)cout, (int)max_workers,
                 cur_stream());
  return y;
}

std::vector<int64_t> conv3x3_plan_py(int64_t n, int64_t h, int64_t w,
                                     int64_t cin, int64_t cout,
                                     int64_t max_workers) {
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
              conv3x3_supported(n, h, w, (int)cin, (int)cout));
  int rows, imgs, tiles, workers;
  conv3x3_plan((int)n, (int)h, (int)w, (int)cin, (int)cout,
               (int)max_workers, &rows, &imgs, &tiles, &workers);
  return {rows, imgs, tiles, workers};
}

// dw [Cout,3,3,Cin] = weight gradient of conv3x3 from x [N,H,W,Cin] and
// dy [N,H,W,Cout]. The per-worker fp32 slabs come from the caching
// allocator and are fully written by the launch: no memset, no host
// synchronisation, capturable.
at::Tensor conv3x3_wgrad(const at::Tensor& x, const at::Tensor& dy,
                         int64_t max_workers) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(dy);
  TORCH_CHECK(dy.device() == x.device(),
              "conv3x3_wgrad: x and dy must share one device");
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4,
              "conv3x3_wgrad takes x as [N,H,W,Cin] and dy as [N,H,W,Cout]");
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == x.size(1) &&
                  dy.size(2) == x.size(2),
              "conv3x3_wgrad: x ", x.sizes(), " and dy ", dy.sizes(),
              " must agree in N, H and W");
  const int64_t n = x.size(0), h = x.size(1), w = x.size(2);
  const int64_t cin = x.size(3), cout = dy.size(3);
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
                  conv3x3_supported(n, h, w, (int)cin, (int)cout),
              "conv3x3_wgrad requires Cin and Cout multiples of 64,"
              " 1 <= W <= 56, H >= 1 and N*H*W < 2^31, got x ", x.sizes(),
              " dy ", dy.sizes());
  TORCH_CHECK(max_workers >= 0 && max_workers < (1 << 20));
  DeviceGuard guard(x.device());
  int rows, imgs, tiles, workers;
  conv3x3_wgrad_plan((int)n, (int)h, (int)w, (int)cin, (int)cout,
                     (int)max_workers, &rows, &imgs, &tiles, &workers);
  auto slabs = at::empty({workers, cout * 9 * cin},
                         x.options().dtype(at::kFloat));
  auto dw = at::empty({cout, 3, 3, cin}, x.options());
  launch_conv3x3_wgrad(bf_ptr(x), bf_ptr(dy), slabs.data_ptr<float>(),
                       bf_ptr_mut(dw), (int)n, (int)h, (int)w, (int)cin,
                       (int)cout, (int)max_workers, cur_stream());
  return dw;
}

std::vector<int64_t> conv3x3_wgrad_plan_py(int64_t n, int64_t h, int64_t w,
                                           int64_t cin, int64_t cout,
                                           int64_t max_workers) {
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
              conv3x3_supported(n, h, w, (int)cin, (int)cout));
  int rows, imgs, tiles, workers;
  conv3x3_wgrad_plan((int)n, (int)h, (int)w, (int)cin, (int)cout,
                     (int)max_workers, &rows, &imgs, &tiles, &workers);
  return {rows, imgs, tiles, workers};
}

// ---------------------------------------------------------------------
// 3x3 stride-2 pad-1 convolution, NHWC bf16
// ---------------------------------------------------------------------

// y [N,Ho,Wo,Cout] = conv3x3 at stride 2 of x [N,H,W,Cin] with
// wt [Cout,3,3,Cin], zero padding, no bias.
at::Tensor conv3x3_s2(const at::Tensor& x, const at::Tensor& wt,
                      int64_t max_workers) {
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(wt);
  TORCH_CHECK(wt.device() == x.device(),
              "conv3x3_s2: x and wt must share one device");
  TORCH_CHECK(x.dim() == 4 && wt.dim() == 4,
              "conv3x3_s2 takes x as [N,H,W,Cin] and wt as [Cout,3,3,Cin]");
  TORCH_CHECK(wt.size(3) == x.size(3), "conv3x3_s2: x has ", x.size(3),
              " input channels, wt has ", wt.size(3));
  TORCH_CHECK(wt.size(1) == 3 && wt.size(2) == 3,
              "conv3x3_s2 takes 3x3 taps, got ", wt.size(1), "x", wt.size(2));
  const int64_t n = x.size(0), h = x.size(1), w = x.size(2);
  const int64_t cin = x.size(3), cout = wt.size(0);
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
                  conv3x3_s2_supported(n, h, w, (int)cin, (int)cout),
              "conv3x3_s2 requires Cin and Cout multiples of 64,"
              " 1 <= W <= 56, H >= 1 and N*H*W < 2^31, got x ", x.sizes(),
              " wt ", wt.sizes());
  TORCH_CHECK(max_workers >= 0 && max_workers < (1 << 20));
  DeviceGuard guard(x.device());
  auto y = at::empty({n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, cout},
                     x.options());
  launch_conv3x3_s2(bf_ptr(x), bf_ptr(wt), bf_ptr_mut(y), (int)n, (int)h,
                    (int)w, (int)cin, (int)cout, (int)max_workers,
                    cur_stream());
  return y;
}

// dx [N,h,w,Cin] = data gradient of that convolution from
// dy [N,Ho,Wo,Cout] and wd [Cin,3,3,Cout] (unflipped).
at::Tensor conv3x3_s2_dgrad(const at::Tensor& dy, const at::Tensor& wd,
                            int64_t h, int64_t w, int64_t max_workers) {
  CHECK_BF16_CUDA(dy);
  CHECK_BF16_CUDA(wd);
  TORCH_CHECK(wd.device() == dy.device(),
              "conv3x3_s2_dgrad: dy and wd must share one device");
  TORCH_CHECK(dy.dim() == 4 && wd.dim() == 4,
              "conv3x3_s2_dgrad takes dy as [N,Ho,Wo,Cout] and wd as "
              "[Cin,3,3,Cout]");
  TORCH_CHECK(wd.size(3) == dy.size(3), "conv3x3_s2_dgrad: dy has ",
              dy.size(3), " channels, wd has ", wd.size(3));
  TORCH_CHECK(wd.size(1) == 3 && wd.size(2) == 3,
              "conv3x3_s2_dgrad takes 3x3 taps, got ", wd.size(1), "x",
              wd.size(2));
  const int64_t n = dy.size(0), cout = dy.size(3), cin = wd.size(0);
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
                  conv3x3_s2_supported(n, h, w, (int)cin, (int)cout),
              "conv3x3_s2_dgrad requires Cin and Cout multiples of 64,"
              " 1 <= W <= 56, H >= 1 and N*H*W < 2^31, got dy ", dy.sizes(),
              " wd ", wd.sizes(), " h ", h, " w ", w);
  TORCH_CHECK(dy.size(1) == (h - 1) / 2 + 1 && dy.size(2) == (w - 1) / 2 + 1,
              "conv3x3_s2_dgrad: dy ", dy.sizes(),
              " is not the output of an input of ", h, "x", w);
  TORCH_CHECK(max_workers >= 0 && max_workers < (1 << 20));
  DeviceGuard guard(dy.device());
  auto dx = at::empty({n, h, w, cin}, dy.options());
  launch_conv3x3_s2_dgrad(bf_ptr(dy), bf_ptr(wd), bf_ptr_mut(dx), (int)n,
                          (int)h, (int)w, (int)cin, (int)cout,
                          (int)max_workers, cur_stream());
  return dx;
}

std::vector<int64_t> conv3x3_s2_plan_py(int64_t n, int64_t h, int64_t w,
                                        int64_t cin, int64_t cout,
                                        int64_t max_workers) {
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
              conv3x3_s2_supported(n, h, w, (int)cin, (int)cout));
  int rows, imgs, tiles, workers;
  conv3x3_s2_plan((int)n, (int)h, (int)w, (int)cin, (int)cout,
                  (int)max_workers, &rows, &imgs, &tiles, &workers);
  return {rows, imgs, tiles, workers};
}

std::vector<int64_t> conv3x3_s2_dgrad_plan_py(int64_t n, int64_t h, int64_t w,
                                              int64_t cin, int64_t cout,
                                              int64_t max_workers) {
  TORCH_CHECK(cin < (1 << 20) && cout < (1 << 20) &&
              conv3x3_s2_supported(n, h, w, (int)cin, (int)cout));
  int rows, imgs, tiles, workers;
  conv3x3_s2_dgrad_plan((int)n, (int)h, (int)w, (int)cin, (int)cout,
                        (int)max_workers, &rows, &imgs, &tiles, &workers);
  return {rows, imgs, tiles, workers};
}

// ---------------------------------------------------------------------
// Flash attention (D=64 and D=128)
// ---------------------------------------------------------------------

static const long long* seed_ptr(const c10::optional<at::Tensor>& seed) {
  if (!seed.has_value()) return nullptr;
  TORCH_CHECK(seed->is_cuda() && seed->scalar_type() == at::kLong &&
              seed->numel() >= 1);
  return reinterpret_cast<const long long*>(seed->data_ptr<int64_t>());
}

// Per-sequence lengths of a right-padded batch: int32 on the data's
// device, one entry per batch row (`rows` = B for the packed layout, BH
// for plain [BH,S,D]). The VALUES stay on the device (the kernels
// clamp them into [0,S]); only the metadata is validated here.
static const int* seqlens_ptr(const c10::optional<at::Tensor>& seqlens,
                              const at::Tensor& like, int64_t rows) {
  if (!seqlens.has_value()) return nullptr;
  TORCH_CHECK(seqlens->is_cuda(), "seqlens must be on GPU");
  TORCH_CHECK(seqlens->device() == like.device(),
              "seqlens must be on the same device as the data");
  TORCH_CHECK(seqlens->scalar_type() == at::kInt,
              "seqlens must be int32");
  TORCH_CHECK(seqlens->is_contiguous(), "seqlens must be contiguous");
  TORCH_CHECK(seqlens->numel() == rows, "seqlens must hold ", rows,
              " entries, got ", seqlens->numel());
  return seqlens->data_ptr<int>();
}

// Head widths with kernels: 64 (attention.hip, attention_causal.hip) and
// 128 (attention_d128.hip).
static bool attn_width_ok(int64_t d) { return d == 64 || d == 128; }

std::vector<at::Tensor> attn_fwd(const at::Tensor& Q, const at::Tensor& K,
                                 const at::Tensor& V, double dropout_p,
                                 const c10::optional<at::Tensor>& seed,
                                 const c10::optional<at::Tensor>& seqlens,
                                 bool causal) {
  CHECK_BF16_CUDA(Q);
  CHECK_BF16_CUDA(K);
  CHECK_BF16_CUDA(V);
  TORCH_CHECK(Q.dim() == 3 && attn_width_ok(Q.size(2)) &&
                  Q.sizes() == K.sizes() && Q.sizes() == V.sizes(),
              "attn_fwd expects [BH, S, 64] or [BH, S, 128] bf16 q/k/v");
  const int BH = (int)Q.size(0), S = (int)Q.size(1);
  TORCH_CHECK(S % 64 == 0, "attn_fwd requires S % 64 == 0");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, Q, BH);
  DeviceGuard guard(Q.device());
  auto O = at::empty_like(Q);
  auto LSE = at::empty({BH, S}, Q.options().dtype(at::kFloat));
  if (Q.size(2) == 128) {  // transposes on the LDS read: no scratch
    launch_attn_d128_fwd(bf_ptr(Q), bf_ptr(K), bf_ptr(V), bf_ptr_mut(O),
                         LSE.data_ptr<float>(), seed_ptr(seed), BH, S, 1,
                         128, 128, (float)dropout_p, lens, causal,
                         cur_stream());
    return {O, LSE};
  }
  auto VT = at::empty({BH, 64, S}, Q.options());
  launch_attn_pretranspose(bf_ptr(V), bf_ptr_mut(VT), BH, S, 1, 64,
                           cur_stream());
  launch_attn_fwd(bf_ptr(Q), bf_ptr(K), bf_ptr(VT), bf_ptr_mut(O),
                  LSE.data_ptr<float>(), seed_ptr(seed), BH, S, 1, 64,
                  64, (float)dropout_p, lens, causal, cur_stream());
  return {O, LSE};
}

std::vector<at::Tensor> attn_fwd_packed(
    const at::Tensor& qkv, double dropout_p,
    const c10::optional<at::Tensor>& seed,
    const c10::optional<at::Tensor>& seqlens, bool causal) {
  CHECK_BF16_CUDA(qkv);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3 &&
                  attn_width_ok(qkv.size(4)) && qkv.is_contiguous(),
              "attn_fwd_packed expects contiguous [B,S,3,H,64] or "
              "[B,S,3,H,128] bf16");
  const int B = (int)qkv.size(0), S = (int)qkv.size(1),
            H = (int)qkv.size(3), D = (int)qkv.size(4);
  TORCH_CHECK(S % 64 == 0, "attn requires S % 64 == 0");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value());
  const int* lens = seqlens_ptr(seqlens, qkv, B);
  DeviceGuard guard(qkv.device());
  auto O = at::empty({B, S, H * D}, qkv.options());
  auto LSE = at::empty({B * H, S}, qkv.options().dtype(at::kFloat));
  const short* base = bf_ptr(qkv);
  if (D == 128) {
    launch_attn_d128_fwd(base, base + (long long)H * 128,
                         base + (long long)2 * H * 128, bf_ptr_mut(O),
                         LSE.data_ptr<float>(), seed_ptr(seed), B * H, S, H,
                         3 * H * 128, H * 128, (float)dropout_p, lens,
                         causal, cur_stream());
    return {O, LSE};
  }
  auto VT = at::empty({B * H, 64, S}, qkv.options());
  launch_attn_pretranspose(base + (long long)2 * H * 64, bf_ptr_mut(VT),
                           B * H, S, H, 3 * H * 64, cur_stream());
  launch_attn_fwd(base, base + (long long)H * 64, bf_ptr(VT),
                  bf_ptr_mut(O), LSE.data_ptr<float>(), seed_ptr(seed),
                  B * H, S, H, 3 * H * 64, H * 64, (float)dropout_p, lens,
                  causal, cur_stream());
  return {O, LSE};
}

std::vector<at::Tensor> attn_bwd(const at::Tensor& Q, const at::Tensor& K,
                                 const at::Tensor& V, const at::Tensor& dO,
                                 const at::Tensor& LSE,
                                 const at::Tensor& Drow, double dropout_p,
                                 const c10::optional<at::Tensor>& seed,
                                 const c10::optional<at::Tensor>& seqlens,
                                 bool causal) {
  CHECK_BF16_CUDA(Q);
  CHECK_BF16_CUDA(K);
  CHECK_BF16_CUDA(V);
  CHECK_BF16_CUDA(dO);
  CHECK_F32_CUDA(LSE);
  CHECK_F32_CUDA(Drow);
  // same shape contract as attn_fwd: the kernels index every operand
  // with Q's [BH, S, D] extents
  TORCH_CHECK(Q.dim() == 3 && attn_width_ok(Q.size(2)) &&
                  Q.sizes() == K.sizes() && Q.sizes() == V.sizes() &&
                  Q.sizes() == dO.sizes(),
              "attn_bwd expects [BH, S, 64] or [BH, S, 128] bf16 q/k/v/dO "
              "of equal sizes");
  const int BH = (int)Q.size(0), S = (int)Q.size(1);
  TORCH_CHECK(S % 64 == 0, "attn_bwd requires S % 64 == 0");
  TORCH_CHECK(LSE.dim() == 2 && LSE.size(0) == BH && LSE.size(1) == S &&
                  LSE.sizes() == Drow.sizes(),
              "attn_bwd expects [BH, S] fp32 LSE and Drow");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, Q, BH);
  DeviceGuard guard(Q.device());
  auto dQ = at::empty_like(Q);
  auto dK = at::empty_like(K);
  auto dV = at::empty_like(V);
  if (Q.size(2) == 128) {
    launch_attn_d128_bwd(bf_ptr(Q), bf_ptr(K), bf_ptr(V), bf_ptr(dO),
                         LSE.data_ptr<float>(), Drow.data_ptr<float>(),
                         bf_ptr_mut(dQ), bf_ptr_mut(dK), bf_ptr_mut(dV),
                         seed_ptr(seed), BH, S, 1, 128, 128, 128,
                         (float)dropout_p, lens, causal, cur_stream());
    return {dQ, dK, dV};
  }
  auto T3 = at::empty({3, BH, 64, S}, Q.options());
  short* qt = bf_ptr_mut(T3);
  short* dot = qt + (long long)BH * 64 * S;
  short* ktt = dot + (long long)BH * 64 * S;
  launch_attn_pretranspose(bf_ptr(Q), qt, BH, S, 1, 64, cur_stream());
  launch_attn_pretranspose(bf_ptr(dO), dot, BH, S, 1, 64, cur_stream());
  launch_attn_pretranspose(bf_ptr(K), ktt, BH, S, 1, 64, cur_stream());
  launch_attn_bwd(bf_ptr(Q), bf_ptr(K), bf_ptr(V), bf_ptr(dO), qt, dot,
                  ktt, LSE.data_ptr<float>(), Drow.data_ptr<float>(),
                  bf_ptr_mut(dQ), bf_ptr_mut(dK), bf_ptr_mut(dV),
                  seed_ptr(seed), BH, S, 1, 64, 64, 64, (float)dropout_p,
                  lens, causal, cur_stream());
  return {dQ, dK, dV};
}

at::Tensor attn_bwd_packed(const at::Tensor& qkv, const at::Tensor& dO,
                           const at::Tensor& LSE, const at::Tensor& Drow,
                           double dropout_p,
                           const c10::optional<at::Tensor>& seed,
                           const c10::optional<at::Tensor>& seqlens,
                           bool causal) {
  CHECK_BF16_CUDA(qkv);
  CHECK_BF16_CUDA(dO);
  CHECK_F32_CUDA(LSE);
  CHECK_F32_CUDA(Drow);
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3 &&
                  attn_width_ok(qkv.size(4)),
              "attn_bwd_packed expects contiguous [B,S,3,H,64] or "
              "[B,S,3,H,128] bf16");
  const int B = (int)qkv.size(0), S = (int)qkv.size(1),
            H = (int)qkv.size(3), D = (int)qkv.size(4);
  TORCH_CHECK(S % 64 == 0, "attn requires S % 64 == 0");
  TORCH_CHECK(dO.dim() == 3 && dO.size(0) == B && dO.size(1) == S &&
                  dO.size(2) == (int64_t)H * D,
              "attn_bwd_packed expects dO [B, S, H*64] or [B, S, H*128]");
  TORCH_CHECK(LSE.dim() == 2 && LSE.size(0) == (int64_t)B * H &&
                  LSE.size(1) == S && LSE.sizes() == Drow.sizes(),
              "attn_bwd_packed expects [B*H, S] fp32 LSE and Drow");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, qkv, B);
  DeviceGuard guard(qkv.device());
  auto dqkv = at::empty_like(qkv);
  const short* base = bf_ptr(qkv);
  short* gbase = bf_ptr_mut(dqkv);
  const int BH = B * H;
  if (D == 128) {
    launch_attn_d128_bwd(base, base + (long long)H * 128,
                         base + (long long)2 * H * 128, bf_ptr(dO),
                         LSE.data_ptr<float>(), Drow.data_ptr<float>(),
                         gbase, gbase + (long long)H * 128,
                         gbase + (long long)2 * H * 128, seed_ptr(seed), BH,
                         S, H, 3 * H * 128, H * 128, 3 * H * 128,
                         (float)dropout_p, lens, causal, cur_stream());
    return dqkv;
  }
  auto T3 = at::empty({3, BH, 64, S}, qkv.options());
  short* qt = bf_ptr_mut(T3);
  short* dot = qt + (long long)BH * 64 * S;
  short* ktt = dot + (long long)BH * 64 * S;
  launch_attn_pretranspose(base, qt, BH, S, H, 3 * H * 64, cur_stream());
  launch_attn_pretranspose(bf_ptr(dO), dot, BH, S, H, H * 64,
                           cur_stream());
  launch_attn_pretranspose(base + (long long)H * 64, ktt, BH, S, H,
                           3 * H * 64, cur_stream());
  launch_attn_bwd(base, base + (long long)H * 64,
                  base + (long long)2 * H * 64, bf_ptr(dO), qt, dot, ktt,
                  LSE.data_ptr<float>(), Drow.data_ptr<float>(), gbase,
                  gbase + (long long)H * 64,
                  gbase + (long long)2 * H * 64, seed_ptr(seed), BH, S,
                  H, 3 * H * 64, H * 64, 3 * H * 64, (float)dropout_p,
                  lens, causal, cur_stream());
  return dqkv;
}

// Grouped-query attention (attention_gqa.hip), 128-wide heads. Every
// extent the kernels index with is checked here, before any launch.
static void attn_gqa_check_heads(int64_t Hq, int64_t Hkv, int64_t S,
                                 int64_t B, const char* who) {
  TORCH_CHECK(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0, who, ": Hkv = ", Hkv,
              " must divide Hq = ", Hq);
  TORCH_CHECK(S >= 64 && S % 64 == 0 && S / 64 <= 65535, who,
              " requires S % 64 == 0, 64 <= S <= 65535 * 64, got ", S);
  TORCH_CHECK(B >= 1 && B * Hq < (int64_t(1) << 31) / S, who,
              ": B * Hq * S must stay below 2^31");
}

// q/dO [B*Hq,S,128], k/v [B*Hkv,S,128] -> B
static int attn_gqa_check_qkv(const at::Tensor& Q, const at::Tensor& K,
                              const at::Tensor& V, int64_t Hq, int64_t Hkv,
                              const char* who) {
  CHECK_BF16_CUDA(Q);
  CHECK_BF16_CUDA(K);
  CHECK_BF16_CUDA(V);
  TORCH_CHECK(Q.dim() == 3 && K.dim() == 3 && Q.size(2) == 128 &&
                  K.size(2) == 128 && K.sizes() == V.sizes() &&
                  Q.size(1) == K.size(1),
              who, " expects bf16 q [B*Hq, S, 128] and k, v [B*Hkv, S, 128]");
  TORCH_CHECK(K.device() == Q.device() && V.device() == Q.device(), who,
              ": all tensors on one device");
  TORCH_CHECK(Hq >= 1 && Hkv >= 1 && Q.size(0) % Hq == 0 &&
                  K.size(0) == Q.size(0) / Hq * Hkv,
              who, ": q holds ", Q.size(0), " heads and k ", K.size(0),
              ", not B*", Hq, " and B*", Hkv);
  attn_gqa_check_heads(Hq, Hkv, Q.size(1), Q.size(0) / Hq, who);
  return (int)(Q.size(0) / Hq);
}

static void attn_gqa_check_bwd(const at::Tensor& LSE, const at::Tensor& Drow,
                               const at::Tensor& like, int64_t BHq,
                               int64_t S, const char* who) {
  CHECK_F32_CUDA(LSE);
  CHECK_F32_CUDA(Drow);
  TORCH_CHECK(LSE.dim() == 2 && LSE.size(0) == BHq && LSE.size(1) == S &&
                  LSE.sizes() == Drow.sizes(),
              who, " expects [B*Hq, S] fp32 LSE and Drow");
  TORCH_CHECK(LSE.device() == like.device() &&
                  Drow.device() == like.device(),
              who, ": all tensors on one device");
}

std::vector<at::Tensor> attn_gqa_fwd(
    const at::Tensor& Q, const at::Tensor& K, const at::Tensor& V,
    double dropout_p, const c10::optional<at::Tensor>& seed,
    const c10::optional<at::Tensor>& seqlens, bool causal, int64_t Hq,
    int64_t Hkv) {
  const int B = attn_gqa_check_qkv(Q, K, V, Hq, Hkv, "attn_gqa_fwd");
  const int S = (int)Q.size(1);
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, Q, B);
  DeviceGuard guard(Q.device());
  auto O = at::empty_like(Q);
  auto LSE = at::empty({Q.size(0), S}, Q.options().dtype(at::kFloat));
  launch_attn_gqa_fwd(bf_ptr(Q), bf_ptr(K), bf_ptr(V), bf_ptr_mut(O),
                      LSE.data_ptr<float>(), seed_ptr(seed), B, S, (int)Hq,
                      (int)Hkv, false, (float)dropout_p, lens, causal,
                      cur_stream());
  return {O, LSE};
}

std::vector<at::Tensor> attn_gqa_bwd(
    const at::Tensor& Q, const at::Tensor& K, const at::Tensor& V,
    const at::Tensor& dO, const at::Tensor& LSE, const at::Tensor& Drow,
    double dropout_p, const c10::optional<at::Tensor>& seed,
    const c10::optional<at::Tensor>& seqlens, bool causal, int64_t Hq,
    int64_t Hkv) {
  const int B = attn_gqa_check_qkv(Q, K, V, Hq, Hkv, "attn_gqa_bwd");
  const int S = (int)Q.size(1);
  CHECK_BF16_CUDA(dO);
  TORCH_CHECK(dO.sizes() == Q.sizes() && dO.device() == Q.device(),
              "attn_gqa_bwd expects dO shaped as q, on q's device");
  attn_gqa_check_bwd(LSE, Drow, Q, Q.size(0), S, "attn_gqa_bwd");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, Q, B);
  DeviceGuard guard(Q.device());
  auto dQ = at::empty_like(Q);
  auto dK = at::empty_like(K);
  auto dV = at::empty_like(V);
  launch_attn_gqa_bwd(bf_ptr(Q), bf_ptr(K), bf_ptr(V), bf_ptr(dO),
                      LSE.data_ptr<float>(), Drow.data_ptr<float>(),
                      bf_ptr_mut(dQ), bf_ptr_mut(dK), bf_ptr_mut(dV),
                      seed_ptr(seed), B, S, (int)Hq, (int)Hkv, false,
                      (float)dropout_p, lens, causal, cur_stream());
  return {dQ, dK, dV};
}

// qkv [B,S,Hq+2Hkv,128]: heads 0..Hq-1 are Q, then Hkv K heads, then Hkv
// V heads (one fused projection's output)
static void attn_gqa_check_packed(const at::Tensor& qkv, int64_t Hq,
                                  int64_t Hkv, const char* who) {
  CHECK_BF16_CUDA(qkv);
  TORCH_CHECK(qkv.dim() == 4 && qkv.size(3) == 128, who,
              " expects contiguous [B, S, Hq + 2*Hkv, 128] bf16");
  TORCH_CHECK(Hq >= 1 && Hkv >= 1 && qkv.size(2) == Hq + 2 * Hkv, who,
              ": qkv holds ", qkv.size(2), " heads, not ", Hq, " + 2*", Hkv);
  attn_gqa_check_heads(Hq, Hkv, qkv.size(1), qkv.size(0), who);
  TORCH_CHECK(qkv.size(0) < (int64_t(1) << 31) / (qkv.size(1) * qkv.size(2)),
              who, ": B * S * (Hq + 2*Hkv) must stay below 2^31");
}

std::vector<at::Tensor> attn_gqa_fwd_packed(
    const at::Tensor& qkv, double dropout_p,
    const c10::optional<at::Tensor>& seed,
    const c10::optional<at::Tensor>& seqlens, bool causal, int64_t Hq,
    int64_t Hkv) {
  attn_gqa_check_packed(qkv, Hq, Hkv, "attn_gqa_fwd_packed");
  const int B = (int)qkv.size(0), S = (int)qkv.size(1);
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, qkv, B);
  DeviceGuard guard(qkv.device());
  auto O = at::empty({B, S, Hq * 128}, qkv.options());
  auto LSE = at::empty({B * Hq, S}, qkv.options().dtype(at::kFloat));
  const short* base = bf_ptr(qkv);
  launch_attn_gqa_fwd(base, base + Hq * 128, base + (Hq + Hkv) * 128,
                      bf_ptr_mut(O), LSE.data_ptr<float>(), seed_ptr(seed),
                      B, S, (int)Hq, (int)Hkv, true, (float)dropout_p, lens,
                      causal, cur_stream());
  return {O, LSE};
}

at::Tensor attn_gqa_bwd_packed(const at::Tensor& qkv, const at::Tensor& dO,
                               const at::Tensor& LSE, const at::Tensor& Drow,
                               double dropout_p,
                               const c10::optional<at::Tensor>& seed,
                               const c10::optional<at::Tensor>& seqlens,
                               bool causal, int64_t Hq, int64_t Hkv) {
  attn_gqa_check_packed(qkv, Hq, Hkv, "attn_gqa_bwd_packed");
  const int B = (int)qkv.size(0), S = (int)qkv.size(1);
  CHECK_BF16_CUDA(dO);
  TORCH_CHECK(dO.dim() == 3 && dO.size(0) == B && dO.size(1) == S &&
                  dO.size(2) == Hq * 128 && dO.device() == qkv.device(),
              "attn_gqa_bwd_packed expects dO [B, S, Hq*128] on qkv's "
              "device");
  attn_gqa_check_bwd(LSE, Drow, qkv, (int64_t)B * Hq, S,
                     "attn_gqa_bwd_packed");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int* lens = seqlens_ptr(seqlens, qkv, B);
  DeviceGuard guard(qkv.device());
  auto dqkv = at::empty_like(qkv);
  const short* base = bf_ptr(qkv);
  short* gbase = bf_ptr_mut(dqkv);
  launch_attn_gqa_bwd(base, base + Hq * 128, base + (Hq + Hkv) * 128,
                      bf_ptr(dO), LSE.data_ptr<float>(),
                      Drow.data_ptr<float>(), gbase, gbase + Hq * 128,
                      gbase + (Hq + Hkv) * 128, seed_ptr(seed), B, S,
                      (int)Hq, (int)Hkv, true, (float)dropout_p, lens,
                      causal, cur_stream());
  return dqkv;
}

// Unpadded attention (attention_unpad.hip): the checks shared by forward
// and backward, and the tile schedule built from cu_seqlens on the device.
static at::Tensor attn_unpad_schedule(const at::Tensor& qkv,
                                      const at::Tensor& cu_seqlens,
                                      const char* who) {
  CHECK_BF16_CUDA(qkv);
  TORCH_CHECK(qkv.dim() == 4 && qkv.size(1) == 3 &&
                  attn_width_ok(qkv.size(3)) && qkv.is_contiguous(),
              who, " expects contiguous [T,3,H,64] or [T,3,H,128] bf16");
  TORCH_CHECK(qkv.size(0) >= 1, who, " expects at least one token");
  TORCH_CHECK(qkv.size(0) < (int64_t(1) << 31) /
                                (3 * qkv.size(2) * qkv.size(3)),
              who, ": T * 3 * H * D must stay below 2^31");
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.device() == qkv.device(),
              "cu_seqlens must be on the same GPU as the data");
  TORCH_CHECK(cu_seqlens.scalar_type() == at::kInt,
              "cu_seqlens must be int32");
  TORCH_CHECK(cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.is_contiguous(),
              "cu_seqlens must be one-dimensional [B+1], B >= 1");
  const int T = (int)qkv.size(0), B = (int)cu_seqlens.numel() - 1;
  DeviceGuard guard(qkv.device());
  auto sched = at::empty({1 + attn_unpad_max_tiles(T, B), 4},
                         cu_seqlens.options());
  launch_attn_unpad_schedule(cu_seqlens.data_ptr<int>(), B, T,
                             sched.data_ptr<int>(), cur_stream());
  return sched;
}

std::vector<at::Tensor> attn_fwd_unpad(
    const at::Tensor& qkv, const at::Tensor& cu_seqlens, int64_t max_seqlen,
    double dropout_p, const c10::optional<at::Tensor>& seed, bool causal) {
  auto sched = attn_unpad_schedule(qkv, cu_seqlens, "attn_fwd_unpad");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen < (int64_t(1) << 31),
              "max_seqlen out of range");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  const int T = (int)qkv.size(0), H = (int)qkv.size(2),
            D = (int)qkv.size(3), B = (int)cu_seqlens.numel() - 1;
  DeviceGuard guard(qkv.device());
  auto O = at::empty({T, H * D}, qkv.options());
  auto LSE = at::empty({H, T}, qkv.options().dtype(at::kFloat));
  launch_attn_unpad_fwd(bf_ptr(qkv), bf_ptr_mut(O), LSE.data_ptr<float>(),
                        seed_ptr(seed), sched.data_ptr<int>(), B, T, H, D,
                        (int)max_seqlen, (float)dropout_p, causal,
                        cur_stream());
  return {O, LSE};
}

at::Tensor attn_bwd_unpad(const at::Tensor& qkv, const at::Tensor& dO,
                          const at::Tensor& O, const at::Tensor& LSE,
                          const at::Tensor& cu_seqlens, int64_t max_seqlen,
                          double dropout_p,
                          const c10::optional<at::Tensor>& seed,
                          bool causal) {
  auto sched = attn_unpad_schedule(qkv, cu_seqlens, "attn_bwd_unpad");
  CHECK_BF16_CUDA(dO);
  CHECK_BF16_CUDA(O);
  CHECK_F32_CUDA(LSE);
  const int T = (int)qkv.size(0), H = (int)qkv.size(2),
            D = (int)qkv.size(3), B = (int)cu_seqlens.numel() - 1;
  TORCH_CHECK(dO.dim() == 2 && dO.size(0) == T &&
                  dO.size(1) == (int64_t)H * D && dO.is_contiguous() &&
                  O.sizes() == dO.sizes() && O.is_contiguous(),
              "attn_bwd_unpad expects contiguous dO and O [T, H*D]");
  TORCH_CHECK(LSE.dim() == 2 && LSE.size(0) == H && LSE.size(1) == T &&
                  LSE.is_contiguous(),
              "attn_bwd_unpad expects contiguous [H, T] fp32 LSE");
  TORCH_CHECK(dO.device() == qkv.device() && O.device() == qkv.device() &&
                  LSE.device() == qkv.device(),
              "attn_bwd_unpad: all tensors on one device");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen < (int64_t(1) << 31),
              "max_seqlen out of range");
  TORCH_CHECK(dropout_p == 0.0 || seed.has_value(),
              "dropout needs a seed tensor");
  DeviceGuard guard(qkv.device());
  auto dqkv = at::empty_like(qkv);
  auto Drow = at::empty_like(LSE);
  launch_attn_unpad_rowdot(bf_ptr(dO), bf_ptr(O), Drow.data_ptr<float>(), T,
                           H, D, cur_stream());
  launch_attn_unpad_bwd(bf_ptr(qkv), bf_ptr(dO), LSE.data_ptr<float>(),
                        Drow.data_ptr<float>(), bf_ptr_mut(dqkv),
                        seed_ptr(seed), sched.data_ptr<int>(), B, T, H, D,
                        (int)max_seqlen, (float)dropout_p, causal,
                        cur_stream());
  return dqkv;
}

at::Tensor wgrad_splitk(const at::Tensor& dZ, const at::Tensor& X) {
  CHECK_BF16_CUDA(dZ);
  CHECK_BF16_CUDA(X);
  TORCH_CHECK(dZ.dim() == 2 && X.dim() == 2 && dZ.size(0) == X.size(0));
  const long long M = dZ.size(0);
  const int N = (int)dZ.size(1), K = (int)X.size(1);
  TORCH_CHECK(wgrad_splitk_supported(M, N, K),
              "wgrad_splitk requires N%256==0, K%128==0, M%64==0");
  DeviceGuard guard(dZ.device());
  auto dW = at::empty({N, K}, dZ.options().dtype(at::kFloat));
  launch_wgrad_splitk(bf_ptr(dZ), bf_ptr(X), dW.data_ptr<float>(), M, N,
                      K, cur_stream());
  return dW;
}

at::Tensor transpose_bf16(const at::Tensor& X) {
  CHECK_BF16_CUDA(X);
  TORCH_CHECK(X.dim() == 2 && X.is_contiguous());
  DeviceGuard guard(X.device());
  const int R = (int)X.size(0), C = (int)X.size(1);
  auto Y = at::empty({C, R}, X.options());
  launch_transpose_bf16(bf_ptr(X), bf_ptr_mut(Y), R, C, cur_stream());
  return Y;
}

// ---------------------------------------------------------------------
// Dropout + residual add + LayerNorm (the BERT sublayer tail)
// ---------------------------------------------------------------------

// Shared validation; returns {rows, cols}. a and b are the two bf16
// activations of the call (sub/res forward, h/dy backward).
static std::pair<int, int> dropout_add_ln_check(
    const at::Tensor& a, const at::Tensor& b, const at::Tensor& gamma,
    double p, const c10::optional<at::Tensor>& seed) {
  TORCH_CHECK(a.dim() >= 1 && a.sizes() == b.sizes(),
              "dropout_add_ln: activation shapes differ: ", a.sizes(),
              " vs ", b.sizes());
  TORCH_CHECK(b.device() == a.device() && gamma.device() == a.device(),
              "dropout_add_ln: tensors must share one device");
  TORCH_CHECK(a.numel() > 0 && a.numel() < (int64_t(1) << 31),
              "dropout_add_ln: numel must be in [1, 2^31), got ",
              a.numel());
  const int64_t cols = a.size(-1);
  TORCH_CHECK(gamma.numel() == cols, "dropout_add_ln: gamma has ",
              gamma.numel(), " elements, rows have ", cols);
  TORCH_CHECK(p >= 0.0 && (float)p < 1.f,
              "dropout_add_ln: p must be in [0, 1), "
              "got ", p);
  TORCH_CHECK(p == 0.0 || seed.has_value(),
              "dropout_add_ln: dropout needs a seed tensor");
  if (seed.has_value())
    TORCH_CHECK(seed->device() == a.device(),
                "dropout_add_ln: seed must be on the data's device");
  return {(int)(a.numel() / cols), (int)cols};
}

std::vector<at::Tensor> dropout_add_ln_fwd(
    const at::Tensor& sub, const at::Tensor& res, const at::Tensor& gamma,
    const at::Tensor& beta, double eps, double p,
    const c10::optional<at::Tensor>& seed) {
  CHECK_BF16_CUDA(sub);
  CHECK_BF16_CUDA(res);
  CHECK_F32_CUDA(gamma);
  CHECK_F32_CUDA(beta);
  const auto [rows, cols] = dropout_add_ln_check(sub, res, gamma, p, seed);
  TORCH_CHECK(beta.numel() == cols && beta.device() == sub.device(),
              "dropout_add_ln_fwd: beta must match gamma");
  DeviceGuard guard(sub.device());

  auto y = at::empty_like(sub);
  auto h = at::empty_like(sub);
  auto f32 = sub.options().dtype(at::kFloat);
  auto mean = at::empty({rows}, f32);
  auto rstd = at::empty({rows}, f32);
  launch_dropout_add_ln_fwd(
      bf_ptr(sub), bf_ptr(res), gamma.data_ptr<float>(),
      beta.data_ptr<float>(), bf_ptr_mut(y), bf_ptr_mut(h),
      mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, cols,
      (float)eps, (float)p, p > 0.0 ? seed_ptr(seed) : nullptr,
      cur_stream());
  return {y, h, mean, rstd};
}

// -> {d_sub, d_res, dgamma, dbeta}; with p == 0 d_sub IS d_res.
std::vector<at::Tensor> dropout_add_ln_bwd(
    const at::Tensor& h, const at::Tensor& dy, const at::Tensor& gamma,
    const at::Tensor& mean, const at::Tensor& rstd, double p,
    const c10::optional<at::Tensor>& seed) {
  CHECK_BF16_CUDA(h);
  CHECK_BF16_CUDA(dy);
  CHECK_F32_CUDA(gamma);
  CHECK_F32_CUDA(mean);
  CHECK_F32_CUDA(rstd);
  const auto [rows, cols] = dropout_add_ln_check(h, dy, gamma, p, seed);
  TORCH_CHECK(mean.numel() == rows && rstd.numel() == rows,
              "dropout_add_ln_bwd: mean/rstd must hold one value per row");
  TORCH_CHECK(mean.device() == h.device() && rstd.device() == h.device(),
              "dropout_add_ln_bwd: tensors must share one device");
  TORCH_CHECK(cols <= 8192,
              "dropout_add_ln_bwd LDS partials support cols<=8192");
  DeviceGuard guard(h.device());

  auto d_res = at::empty_like(h);
  auto d_sub = p > 0.0 ? at::empty_like(h) : d_res;
  auto f32 = h.options().dtype(at::kFloat);
  const int blocks = layernorm_bwd_part_rows(rows);
  const int ws_rows = blocks * 4;  // one partial row per wave
  auto dgamma_part = at::empty({ws_rows, cols}, f32);
  auto dbeta_part = at::empty({ws_rows, cols}, f32);
  auto dgamma = at::zeros({cols}, f32);
  auto dbeta = at::zeros({cols}, f32);
  if (p > 0.0) {
    launch_dropout_add_ln_bwd(
        bf_ptr(h), bf_ptr(dy), gamma.data_ptr<float>(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), bf_ptr_mut(d_res),
        bf_ptr_mut(d_sub), dgamma_part.data_ptr<float>(),
        dbeta_part.data_ptr<float>(), blocks, rows, cols, (float)p,
        seed_ptr(seed), cur_stream());
  } else {
    launch_layernorm_bwd(bf_ptr(h), bf_ptr(dy), gamma.data_ptr<float>(),
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),
                         bf_ptr_mut(d_res), dgamma_part.data_ptr<float>(),
                         dbeta_part.data_ptr<float>(), blocks, rows, cols,
                         cur_stream());
  }
  launch_layernorm_reduce_parts(
      dgamma_part.data_ptr<float>(), dbeta_part.data_ptr<float>(),
      dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), ws_rows, cols,
      cur_stream());
  return {d_sub, d_res, dgamma, dbeta};
}

// ---------------------------------------------------------------------
// GBT histogram
// ---------------------------------------------------------------------

at::Tensor gbt_histogram(const at::Tensor& B, const at::Tensor& g,
                         const at::Tensor& h, const at::Tensor& row_list,
                         const at::Tensor& bmap, int64_t n_nodes) {
  TORCH_CHECK(B.is_cuda() && B.scalar_type() == at::kByte &&
              B.is_contiguous());
  CHECK_F32_CUDA(g);
  CHECK_F32_CUDA(h);
  TORCH_CHECK(row_list.is_cuda() && row_list.scalar_type() == at::kInt);
  TORCH_CHECK(bmap.is_cuda() && bmap.scalar_type() == at::kInt &&
              bmap.size(-1) == 4);
  DeviceGuard guard(B.device());
  const int F = (int)B.size(1);
  TORCH_CHECK(F % 8 == 0, "feature dim must be padded to a multiple of 8");
  auto hist = at::zeros({n_nodes, F, 256, 2},
                        B.options().dtype(at::kFloat));
  launch_gbt_histogram(
      B.data_ptr<unsigned char>(), g.data_ptr<float>(),
      h.data_ptr<float>(), row_list.data_ptr<int>(),
      reinterpret_cast<const int4*>(bmap.data_ptr<int>()),
      (int)(bmap.numel() / 4), F, hist.data_ptr<float>(), cur_stream());
  return hist;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "sparkdl MI355X-native kernels (gfx950)";
  m.def("fused_adamw_", &fused_adamw_, "Fused multi-tensor AdamW step");
  m.def("fused_sgd_", &fused_sgd_, "Fused multi-tensor SGD step");
  m.def("zero_grads_", &zero_grads_, "Zero all grads in a chunk table");
  m.def("gemm_bias_act", &gemm_bias_act, "MFMA GEMM + bias(+GELU) (N6)");
  m.def("transpose_bf16", &transpose_bf16, "bf16 2D transpose (dgrad W^T)");
  m.def("lce_forward", &lce_forward,
        "Fused linear + cross-entropy forward -> loss, lse, count",
        py::arg("h"), py::arg("weight"), py::arg("bias"), py::arg("labels"),
        py::arg("ignore_index") = -100, py::arg("reduction") = "none");
  m.def("lce_backward", &lce_backward,
        "Fused linear + cross-entropy backward -> dZ (padded rows), dbias",
        py::arg("h"), py::arg("weight"), py::arg("bias"), py::arg("labels"),
        py::arg("lse"), py::arg("gout"), py::arg("count"),
        py::arg("ignore_index") = -100);
  m.def("gemm_stream", &gemm_stream,
        "Streaming tall-skinny GEMM (1x1 convs)");
  m.def("conv1x1_stats", &conv1x1_stats,
        "Read-once 1x1 conv forward + BatchNorm partial sums -> C, slab",
        py::arg("a"), py::arg("w"), py::arg("max_workers") = 0,
        py::arg("slab") = py::none());
  m.def("conv1x1_stats_plan", &conv1x1_stats_plan_py,
        "(chunks per N-block, slab rows G) of a conv1x1_stats launch",
        py::arg("m"), py::arg("n"), py::arg("k"),
        py::arg("max_workers") = 0);
  m.def("conv3x3", &conv3x3,
        "3x3 stride-1 pad-1 convolution, NHWC bf16 (forward and dgrad)",
        py::arg("x"), py::arg("wt"), py::arg("max_workers") = 0);
  m.def("conv3x3_plan", &conv3x3_plan_py,
        "(rows per band, images per tile, tiles and workers per N-block) "
        "of a conv3x3 launch",
        py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"),
        py::arg("cout"), py::arg("max_workers") = 0);
  m.def("conv3x3_wgrad", &conv3x3_wgrad,
        "Weight gradient [Cout,3,3,Cin] of the 3x3 stride-1 pad-1 "
        "convolution, NHWC bf16, deterministic",
        py::arg("x"), py::arg("dy"), py::arg("max_workers") = 0);
  m.def("conv3x3_wgrad_plan", &conv3x3_wgrad_plan_py,
        "(rows per band, images per tile, tiles and workers per block "
        "pair) of a conv3x3_wgrad launch",
        py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"),
        py::arg("cout"), py::arg("max_workers") = 0);
  m.def("conv3x3_s2", &conv3x3_s2,
        "3x3 stride-2 pad-1 convolution forward, NHWC bf16",
        py::arg("x"), py::arg("wt"), py::arg("max_workers") = 0);
  m.def("conv3x3_s2_plan", &conv3x3_s2_plan_py,
        "(output rows per band, images per tile, tiles and workers per "
        "N-block) of a conv3x3_s2 launch on an input of h x w",
        py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"),
        py::arg("cout"), py::arg("max_workers") = 0);
  m.def("conv3x3_s2_dgrad", &conv3x3_s2_dgrad,
        "Data gradient [N,h,w,Cin] of the 3x3 stride-2 pad-1 convolution "
        "from dy [N,Ho,Wo,Cout] and wd [Cin,3,3,Cout], NHWC bf16",
        py::arg("dy"), py::arg("wd"), py::arg("h"), py::arg("w"),
        py::arg("max_workers") = 0);
  m.def("conv3x3_s2_dgrad_plan", &conv3x3_s2_dgrad_plan_py,
        "(cell rows per band, dy images per tile, tiles and workers per "
        "Cin block) of a conv3x3_s2_dgrad launch for an input of h x w",
        py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"),
        py::arg("cout"), py::arg("max_workers") = 0);
  m.def("bn_fwd_slab", &bn_fwd_slab,
        "Fused BatchNorm(+add)(+ReLU) fwd over pre-summed statistics");
  m.def("wgrad_splitk", &wgrad_splitk,
        "Split-M wgrad GEMM (tr_b16 fragment path)");
  // trailing seqlens defaults to None and causal to false, so the
  // shorter positional calls from before either argument keep working
  m.def("attn_fwd", &attn_fwd, "Flash attention fwd (D=64 or 128, bf16)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dropout_p"),
        py::arg("seed"), py::arg("seqlens") = py::none(),
        py::arg("causal") = false);
  m.def("attn_bwd", &attn_bwd, "Flash attention bwd (dQ/dK/dV)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dO"),
        py::arg("lse"), py::arg("drow"), py::arg("dropout_p"),
        py::arg("seed"), py::arg("seqlens") = py::none(),
        py::arg("causal") = false);
  m.def("attn_fwd_packed", &attn_fwd_packed,
        "Flash attention fwd over the packed qkv buffer", py::arg("qkv"),
        py::arg("dropout_p"), py::arg("seed"),
        py::arg("seqlens") = py::none(), py::arg("causal") = false);
  m.def("attn_bwd_packed", &attn_bwd_packed,
        "Flash attention bwd -> packed dqkv", py::arg("qkv"),
        py::arg("dO"), py::arg("lse"), py::arg("drow"),
        py::arg("dropout_p"), py::arg("seed"),
        py::arg("seqlens") = py::none(), py::arg("causal") = false);
  m.def("attn_gqa_fwd", &attn_gqa_fwd,
        "Grouped-query flash attention fwd (D=128): q [B*Hq,S,128], "
        "k/v [B*Hkv,S,128] -> (O, LSE)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dropout_p"),
        py::arg("seed"), py::arg("seqlens"), py::arg("causal"),
        py::arg("num_q_heads"), py::arg("num_kv_heads"));
  m.def("attn_gqa_bwd", &attn_gqa_bwd,
        "Grouped-query flash attention bwd -> (dQ, dK, dV)", py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("dO"), py::arg("lse"),
        py::arg("drow"), py::arg("dropout_p"), py::arg("seed"),
        py::arg("seqlens"), py::arg("causal"), py::arg("num_q_heads"),
        py::arg("num_kv_heads"));
  m.def("attn_gqa_fwd_packed", &attn_gqa_fwd_packed,
        "Grouped-query flash attention fwd over [B,S,Hq+2Hkv,128]",
        py::arg("qkv"), py::arg("dropout_p"), py::arg("seed"),
        py::arg("seqlens"), py::arg("causal"), py::arg("num_q_heads"),
        py::arg("num_kv_heads"));
  m.def("attn_gqa_bwd_packed", &attn_gqa_bwd_packed,
        "Grouped-query flash attention bwd -> packed dqkv", py::arg("qkv"),
        py::arg("dO"), py::arg("lse"), py::arg("drow"),
        py::arg("dropout_p"), py::arg("seed"), py::arg("seqlens"),
        py::arg("causal"), py::arg("num_q_heads"),
        py::arg("num_kv_heads"));
  m.def("attn_fwd_unpad", &attn_fwd_unpad,
        "Flash attention fwd over unpadded [T,3,H,D] qkv -> (O, LSE)",
        py::arg("qkv"), py::arg("cu_seqlens"), py::arg("max_seqlen"),
        py::arg("dropout_p"), py::arg("seed"), py::arg("causal"));
  m.def("attn_bwd_unpad", &attn_bwd_unpad,
        "Flash attention bwd over unpadded qkv -> dqkv", py::arg("qkv"),
        py::arg("dO"), py::arg("o"), py::arg("lse"), py::arg("cu_seqlens"),
        py::arg("max_seqlen"), py::arg("dropout_p"), py::arg("seed"),
        py::arg("causal"));
  m.def("gbt_histogram", &gbt_histogram, "GBT g/h histogram (N7)");
  m.def("bn_fwd", &bn_fwd, "Fused BatchNorm(+add)(+ReLU) fwd (bf16 NHWC)");
  m.def("bn_bwd", &bn_bwd, "Fused BatchNorm(+add)(+ReLU) bwd (bf16 NHWC)");
  m.def("bn_bwd2", &bn_bwd2,
        "Fused BatchNorm(+add)(+ReLU) bwd over the sum of two gradients");
  m.def("bn_pool_fwd", &bn_pool_fwd,
        "Fused BatchNorm+ReLU+MaxPool(3,2,1) fwd (bf16 NHWC)");
  m.def("bn_pool_bwd", &bn_pool_bwd,
        "Fused BatchNorm+ReLU+MaxPool(3,2,1) bwd (bf16 NHWC)");
  m.def("layernorm_fwd", &layernorm_fwd, "LayerNorm forward (bf16)");
  m.def("layernorm_bwd", &layernorm_bwd, "LayerNorm backward (bf16)");
  m.def("dropout_add_ln_fwd", &dropout_add_ln_fwd,
        "ln(res + dropout(sub)) forward (bf16) -> y, h, mean, rstd",
        py::arg("sub"), py::arg("res"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("p"), py::arg("seed") = py::none());
  m.def("dropout_add_ln_bwd", &dropout_add_ln_bwd,
        "ln(res + dropout(sub)) backward -> d_sub, d_res, dgamma, dbeta",
        py::arg("h"), py::arg("dy"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("p"), py::arg("seed") = py::none());
  m.def("bias_gelu_fwd", &bias_gelu_fwd, "Fused bias+GELU forward (bf16)");
  m.def("bias_gelu_bwd", &bias_gelu_bwd, "Fused bias+GELU backward (bf16)");
  m.attr("_chunk_elems") = kOptChunk;
}
