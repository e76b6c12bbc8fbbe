// v3d_api.cpp -- error reporting and version string of libv3d_hip.
#include "v3d_common.h"
#include <string.h>

static thread_local char g_err[512] = "";

void v3d_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* v3d_last_error(void) { return g_err; }
extern "C" const char* v3d_version(void) { return "libv3d_hip 0.2 (gfx950)"; }

v3d_lib_options g_v3d_opt;      // the defaults of V3D_LIB_OPTIONS (v3d_common.h)

extern "C" int v3d_set_option(const char* key, int value)
{
    if (!key) { v3d_set_error("null key"); return V3D_ERR_ARG; }
#define X(name, def, ok, store, doc)                                                                                    \
    if (!strcmp(key, #name)) {                                                                                          \
        if (!(ok)) {                                                                                                    \
            if (!strcmp(key, "gf_cols")) v3d_set_error("option gf_cols: 256 or 512");                                   \
            else v3d_set_error("option %s: value %d out of range", key, value);                                         \
            return V3D_ERR_ARG;                                                                                         \
        }                                                                                                               \
        g_v3d_opt.name = (store);                                                                                       \
        return V3D_OK;                                                                                                  \
    }
    V3D_LIB_OPTIONS(X)
#undef X
    v3d_set_error("unknown option %s", key);
    return V3D_ERR_ARG;
}

extern "C" int v3d_get_option(const char* key, int* value)
{
    if (!key || !value) { v3d_set_error("null argument"); return V3D_ERR_ARG; }
#define X(name, def, ok, store, doc) if (!strcmp(key, #name)) { *value = g_v3d_opt.name; return V3D_OK; }
    V3D_LIB_OPTIONS(X)
#undef X
    v3d_set_error("unknown option %s", key);
    return V3D_ERR_ARG;
}
