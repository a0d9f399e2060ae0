// pt_weighting of the training bases (reference GNNEmbedding/embedding_base.py:95-107; the edge classifier and the
// bipartite bases restate it word for word) in float32, for one pt.  Shared by k_ph_* (pairloss.hip) and k_wb_*
// (wbce.hip).  Q: any struct with the float fields wmin, one_minus_wmin, leak, cut, cap and interval = cap - cut.
#pragma once
#include <hip/hip_runtime.h>

namespace hgnn {

template <class Q>
static __device__ __forceinline__ float ph_ptw(float p, const Q& q) {
    if (p != p) p = 0.f;                                     // embedding_base.py:97
    const float x = p - q.cut, z = p - q.cap;
    float r = (x > 0.f ? 1.f : 0.f) * x / q.interval;        // heaviside(x, 0) * x / (cap - cut)
    r = (r != r) ? r : fminf(r, 1.f);                        // torch.minimum keeps NaN (interval == 0)
    return q.wmin + q.one_minus_wmin * r + q.leak * (z > 0.f ? 1.f : 0.f) * z;
}

}  // namespace hgnn
