// Every process-wide switch of hgnn_set_option (capi.hip; the table of names is in INTEGRATION.md).  Each is
// defined, with its default, in the translation unit that reads it.
#pragma once

namespace hgnn {

extern int g_opt_nt_loads;   // segreduce.hip
extern int g_opt_nt_stores;  // segreduce.hip
extern int g_opt_k1_one_launch;  // segreduce.hip
extern int g_opt_k1_item_order;  // segreduce.hip
#ifdef HGNN_K1_SWEEP         // the sweep library of tools/tune_k1_window.py only
extern int g_opt_k1_window;  // segreduce.hip
extern int g_opt_k1_waves;   // segreduce.hip
#endif
extern int g_opt_mlp_ablate;         // mlp_fused.hip; read by the bf16 MLPs too
extern int g_opt_mlp_act_switch;     // mlp_fused.hip; read by the split-bf16 fp32 MLP too
extern int g_opt_mlp_split_variant;  // mlp_split_bf16.hip
namespace f3 {
extern int g_opt_split3_rows128;  // mlp_split3_f32.hip
extern int g_opt_split3_one_wg;   // mlp_split3_f32.hip
}  // namespace f3

}  // namespace hgnn
