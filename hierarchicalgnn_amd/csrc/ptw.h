// pt_weighting of the training bases (reference GNNEmbedding/embedding_base.py:95-107; the edge classifier and the
// bipartite bases restate it word for word) in float32, for one pt.  Shared by k_ph_* (pairloss.hip) and k_wb_*
// (wbce.hip).  Q: any struct with the float fields wmin, one_minus_wmin, leak, cut, cap and interval = cap - cut.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/hgnn_hip.h"

namespace hgnn {

template <class Q>
static __device__ __forceinline__ float ph_ptw(float p, const Q& q) {
    if (p != p) p = 0.f;                                     // embedding_base.py:97
    const float x = p - q.cut, z = p - q.cap;
    float r = (x > 0.f ? 1.f : 0.f) * x / q.interval;        // heaviside(x, 0) * x / (cap - cut)
    r = (r != r) ? r : fminf(r, 1.f);                        // torch.minimum keeps NaN (interval == 0)
    return q.wmin + q.one_minus_wmin * r + q.leak * (z > 0.f ? 1.f : 0.f) * z;
}

// Q's six fields from the host hparams vector (HGNN_PH_* entries).  interval is cap - cut formed from the double
// cut, as the reference's (cap - cut) is: not pt_interval in floating point.
template <class Q>
void ptw_fill(Q& q, const double* h) {
    q.wmin = (float)h[HGNN_PH_WEIGHT_MIN];
    q.one_minus_wmin = (float)(1.0 - h[HGNN_PH_WEIGHT_MIN]);
    q.leak = (float)h[HGNN_PH_WEIGHT_LEAK];
    q.cut = (float)(h[HGNN_PH_PTCUT] - h[HGNN_PH_PT_INTERVAL]);
    q.cap = (float)h[HGNN_PH_PTCUT];
    q.interval = (float)(h[HGNN_PH_PTCUT] - (h[HGNN_PH_PTCUT] - h[HGNN_PH_PT_INTERVAL]));
}

// the class factors of the loss: sigmoid(lwr) for the true pairs, sigmoid(-lwr) for the false ones
static inline void class_sigmoids(double lwr, double* sig_t, double* sig_f) {
    *sig_t = 1.0 / (1.0 + exp(-lwr));
    *sig_f = 1.0 / (1.0 + exp(lwr));
}

}  // namespace hgnn
