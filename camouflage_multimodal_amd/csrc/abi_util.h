// Host-side vocabulary of the C ABI files (fusion_abi.hip with its workspace layout fusion_ws.h, rg_abi.hip, image_abi.hip,
// seg_measures.hip): the error return, the workspace carver and its check, and the builder of an exact-fp32 GEMM batch.  No device code.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/camo_fusion.h"
#include "gemm.h"

namespace camo_abi {

// Set the calling thread's camo_last_error() string and return the code.  Defined once, in fusion_abi.hip, next to the string; hidden:
// shared between the library's own files, not exported.
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);
__attribute__((visibility("hidden"))) int fail_hip(int e, const char* where);
#define CK(x, where)                                   \
  do {                                                 \
    int e_ = (x);                                      \
    if (e_ != 0) return camo_abi::fail_hip(e_, where); \
  } while (0)

// Hands out consecutive 256-byte aligned pieces of a workspace (null base: sizes only), from `start` on: a layout that continues another's.
struct Carver {
  char* base; size_t off;
  explicit Carver(void* b, size_t start = 0) : base(static_cast<char*>(b)), off(start) {}
  template <typename T> T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  size_t bytes() const { return (off + 255) & ~size_t(255); }      // what has been taken, the last piece rounded up like the others
};

// A caller's workspace `ws` of `ws_bytes` against the `need` bytes that `sizer` (the entry point's ..._workspace_bytes function)
// returns: the alignment first, then the size.
inline int ws_check(const void* ws, size_t ws_bytes, size_t need, const char* sizer) {
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(CAMO_E_ARG, "ws must be 256-byte aligned");
  if (ws_bytes < need) return fail(CAMO_E_ARG, std::string("ws_bytes smaller than ") + sizer + "()");
  return 0;
}

struct GB {
  GemmBatch b;
  GemmProb spill;
  int prec; hipStream_t st;
  GB(const DropCfg& d, int prec_, hipStream_t st_) : prec(prec_), st(st_) { std::memset(&b, 0, sizeof(b)); b.drop = d; }
  GemmProb& add(const float* A, int lda, const float* Bm, int ldb, float* C, int ldc, int M, int N, int K, int flags) {
    // (a 13th problem lands in a spare slot and is counted: launch_gemm_batch refuses the batch, run() reports it)
    GemmProb& p = b.n < GEMM_MAXP ? b.p[b.n] : spill;
    ++b.n;
    std::memset(&p, 0, sizeof(p));   // slots are reused across launches: no stale res/bias_grad/flags
    p.A = A; p.lda = lda; p.B = Bm; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.flags = flags;
    p.aux_scale = 1.f;
    return p;
  }
  // y = x.W^T (+bias): x [M,K], W [N,K]
  GemmProb& nt(const float* x, int ldx, const float* W, int ldw, const float* bias, float* y, int ldy, int M, int N, int K, int flags = 0) {
    GemmProb& p = add(x, ldx, W, ldw, y, ldy, M, N, K, flags);
    p.bias = bias;
    return p;
  }
  // dx = dy.W : dy [M,K=Nout], W [Nout, N=in]
  GemmProb& nn(const float* dy, int lddy, const float* W, int ldw, float* dx, int lddx, int M, int N, int K, int flags = 0) {
    return add(dy, lddy, W, ldw, dx, lddx, M, N, K, flags | GF_B_KMAJOR);
  }
  // dW [Nout, Nin] += dy^T.x : dy [rows, Nout], x [rows, Nin]; db [Nout] += colsum(dy)
  GemmProb& tn(const float* dy, int lddy, const float* x, int ldx, float* dW, int lddw, float* db, int Nout, int Nin, int rows) {
    GemmProb& p = add(dy, lddy, x, ldx, dW, lddw, Nout, Nin, rows, GF_A_KMAJOR | GF_B_KMAJOR | GF_ATOMIC);
    p.bias_grad = db;
    return p;
  }
  int run() {
    if (b.n == 0) return 0;
    int e = launch_gemm_batch(b, prec, st);
    b.n = 0;
    return e;
  }
};
inline void set_relu_bwd(GemmProb& p, const float* act, int ldr, float scale) {
  p.flags |= GF_RELU_BWD; p.res = act; p.ldr = ldr; p.aux_scale = scale;
}

}  // namespace camo_abi
