// Error reporting, version and option entry points of the C ABI (include/hgnn_hip.h).
#include "common.h"
#include "options.h"
#include <climits>
#include <cstdlib>
#include <cstring>

namespace hgnn {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static const struct {
    const char* name;
    int* value;
    int lo, hi;         // accepted range
    const char* takes;  // what the error says when the value is refused
} kOptions[] = {
    {"nt_loads", &g_opt_nt_loads, INT_MIN, INT_MAX, nullptr},
    {"nt_stores", &g_opt_nt_stores, INT_MIN, INT_MAX, nullptr},
    {"k1_one_launch", &g_opt_k1_one_launch, 0, 1, "takes 0 or 1"},
    {"k1_item_order", &g_opt_k1_item_order, 0, 1, "takes 0 or 1"},
#ifdef HGNN_K1_SWEEP
    {"k1_window", &g_opt_k1_window, INT_MIN, INT_MAX, nullptr},
    {"k1_waves", &g_opt_k1_waves, INT_MIN, INT_MAX, nullptr},
#endif
    {"mlp_ablate", &g_opt_mlp_ablate, INT_MIN, INT_MAX, nullptr},  // stored & 31
    {"mlp_act_switch", &g_opt_mlp_act_switch, 0, 1, "takes 0 or 1"},
    {"mlp_split_variant", &g_opt_mlp_split_variant, INT_MIN, INT_MAX, nullptr},
    {"mlp_split3_rows128", &f3::g_opt_split3_rows128, 0, 2,
     "takes 0 or 1 (2 = experimental tile, needs HGNN_EXPERIMENTAL=1)"},
    {"mlp_split3_one_wg", &f3::g_opt_split3_one_wg, INT_MIN, INT_MAX, nullptr},
};
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_abi_version(void) { return HGNN_ABI_VERSION; }
extern "C" const char* hgnn_last_error(void) { return hgnn::g_err; }
extern "C" int hgnn_sizeof_plan(void) { return (int)sizeof(hgnn_plan); }
extern "C" int hgnn_sizeof_mlp_desc(void) { return (int)sizeof(hgnn_mlp_desc); }

extern "C" int hgnn_set_option(const char* name, int value) {
    HGNN_REQUIRE(name != nullptr, "hgnn_set_option: name is NULL");
    for (const auto& o : kOptions) {
        if (strcmp(name, o.name)) continue;
        // mlp_split3_rows128 = 2 is the two-workgroup tile that returned wrong elements in one of two equivalent
        // builds: measurement tools only, behind an environment switch of its own
        const bool experimental = o.value == &f3::g_opt_split3_rows128 && value == 2;
        if (value < o.lo || value > o.hi || (experimental && getenv("HGNN_EXPERIMENTAL") == nullptr)) {
            set_error("hgnn_set_option: %s %s", o.name, o.takes);
            return HGNN_ERR_INVALID_ARG;
        }
        *o.value = o.value == &g_opt_mlp_ablate ? value & 31 : value;
        return HGNN_OK;
    }
    set_error("hgnn_set_option: unknown option '%s'", name);
    return HGNN_ERR_INVALID_ARG;
}

extern "C" int hgnn_get_option(const char* name, int* value) {
    HGNN_REQUIRE(name != nullptr && value != nullptr, "hgnn_get_option: NULL pointer");
    for (const auto& o : kOptions) {
        if (strcmp(name, o.name)) continue;
        *value = *o.value;
        return HGNN_OK;
    }
    set_error("hgnn_get_option: unknown option '%s'", name);
    return HGNN_ERR_INVALID_ARG;
}
