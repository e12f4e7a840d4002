// expr.hip -- derived value columns: an aggregation argument's arithmetic, evaluated once per segment into a doc-order
// value column that every walk then reads as a raw LONG / DOUBLE column (include/pinot_hip.h phip_expr_op;
// runtime.cpp ensure_derived).
//
// The reference evaluates such an argument per block as a chain of double transform functions
// (pinot-core/.../operator/transform/function/AdditionTransformFunction.java, SubtractionTransformFunction.java,
// MultiplicationTransformFunction.java, DivisionTransformFunction.java, LiteralTransformFunction.java): every node
// is one Java double operation, separately rounded. The double instantiation does the same -- __dadd_rn / __dsub_rn /
// __dmul_rn / __ddiv_rn under fp contract(off), so no a * b + c becomes a fused multiply-add. The int64_t
// instantiation uses wrapping integer operations; the host launches it only where the columns' value ranges prove
// that no intermediate leaves int64.
#include "agg_common.h"
#include "launch.h"

namespace phip {

constexpr int kExprBlock = 256;                       // one workgroup per 2048-doc tile
constexpr int kExprLaneDocs = kTileDocs / kExprBlock; // 8 consecutive docs per lane
constexpr int kExprPair = 2;                          // evaluated two at a time: one 16-byte store
static_assert(kExprLaneDocs % kExprPair == 0, "a lane's docs split into 16-byte stores");

typedef const PHIP_CAS DevExpr cexpr_t;
typedef const PHIP_CAS DevExprOp cexop_t;

template <typename T> struct ExprPair;
template <> struct ExprPair<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct ExprPair<int64_t> { typedef int64_t type __attribute__((ext_vector_type(2))); };

template <typename T> __device__ __forceinline__ T expr_load(ccol_t &c, int32_t doc);
template <> __device__ __forceinline__ double expr_load<double>(ccol_t &c, int32_t doc) { return col_f64(c, doc); }
template <> __device__ __forceinline__ int64_t expr_load<int64_t>(ccol_t &c, int32_t doc) { return col_i64(c, doc); }
template <typename T> __device__ __forceinline__ T expr_const(cexop_t &o);
template <> __device__ __forceinline__ double expr_const<double>(cexop_t &o) { return o.dval; }
template <> __device__ __forceinline__ int64_t expr_const<int64_t>(cexop_t &o) { return o.lval; }

#pragma clang fp contract(off)
__device__ __forceinline__ double expr_apply(int op, double a, double b) {
#pragma clang fp contract(off)
  switch (op) {
    case EXOP_ADD: return __dadd_rn(a, b);
    case EXOP_SUB: return __dsub_rn(a, b);
    case EXOP_MUL: return __dmul_rn(a, b);
    default: return __ddiv_rn(a, b);
  }
}
__device__ __forceinline__ int64_t expr_apply(int op, int64_t a, int64_t b) {
  switch (op) {  // (unsigned: wrapping is defined; the host never launches a program with DIV as int64)
    case EXOP_ADD: return (int64_t)((uint64_t)a + (uint64_t)b);
    case EXOP_SUB: return (int64_t)((uint64_t)a - (uint64_t)b);
    default: return (int64_t)((uint64_t)a * (uint64_t)b);
  }
}

// The program is wave-uniform (scalar loads through the constant address space, scalar branches). The value stack's
// top stays in registers; the values below it live in LDS, one column per lane ((kExprMaxStack - 1) x 2 x 256 x 8 B =
// 28 KiB per workgroup): a register array indexed by the stack pointer would go to scratch.
template <typename T>
__global__ __launch_bounds__(kExprBlock) void expr_materialize_kernel(const DevExpr *ep, T *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ T stk[(kExprMaxStack - 1) * kExprPair * kExprBlock];
  cexpr_t &e = *(cexpr_t *)ep;
  const int tid = threadIdx.x;
  const int32_t num_docs = e.num_docs;
  const int32_t num_ops = e.num_ops;
  const int64_t first = (int64_t)blockIdx.x * kTileDocs + (int64_t)tid * kExprLaneDocs;
  if (first >= num_docs) return;  // (the ragged last tile: this lane's docs are all past the end)
  for (int p = 0; p < kExprLaneDocs / kExprPair; p++) {
    const int64_t d0 = first + kExprPair * p, d1 = d0 + 1;
    if (d0 >= num_docs) break;
    // docs past the end read the last doc's inputs (in bounds) and are not stored
    const int32_t l0 = (int32_t)d0, l1 = (int32_t)(d1 < num_docs ? d1 : d0);
    T t0 = 0, t1 = 0;
    int sp = 0;  // values on the stack, the top (t0, t1) included
    for (int i = 0; i < num_ops; i++) {
      cexop_t &o = e.ops[i];
      const int op = o.op;
      if (op <= EXOP_CONST) {
        if (sp > 0) {
          stk[((sp - 1) * kExprPair + 0) * kExprBlock + tid] = t0;
          stk[((sp - 1) * kExprPair + 1) * kExprBlock + tid] = t1;
        }
        if (op == EXOP_COLUMN) {
          ccol_t &c = e.cols[o.col];
          t0 = expr_load<T>(c, l0);
          t1 = expr_load<T>(c, l1);
        } else {
          t0 = t1 = expr_const<T>(o);
        }
        sp++;
      } else {
        sp--;  // (the host validated the program: sp >= 1 here)
        const T a0 = stk[((sp - 1) * kExprPair + 0) * kExprBlock + tid];
        const T a1 = stk[((sp - 1) * kExprPair + 1) * kExprBlock + tid];
        t0 = expr_apply(op, a0, t0);
        t1 = expr_apply(op, a1, t1);
      }
    }
    if (d1 < num_docs) {
      typename ExprPair<T>::type v;
      v.x = t0;
      v.y = t1;
      *(typename ExprPair<T>::type *)(out + d0) = v;  // d0 is even: 16-byte aligned
    } else {
      out[d0] = t0;
    }
  }
}

static hipError_t launch_expr_materialize(const DevExpr *e, int32_t num_docs, bool integral, void *out, hipStream_t s) {
  if (num_docs <= 0) return hipSuccess;
  const int blocks = (int)(((int64_t)num_docs + kTileDocs - 1) / kTileDocs);
  if (integral) expr_materialize_kernel<int64_t><<<blocks, kExprBlock, 0, s>>>(e, (int64_t *)out);
  else expr_materialize_kernel<double><<<blocks, kExprBlock, 0, s>>>(e, (double *)out);
  return hipGetLastError();
}

namespace {
struct ExprRegistration {
  ExprRegistration() { register_expr_launcher(&launch_expr_materialize); }
} g_expr_registration;
}  // namespace

}  // namespace phip
