/*
 * icw_graph_compile.h -- internal: the DSP-list compiler and the render constants
 * (icw_graph_compile.cpp).  Host arithmetic only: no HIP type, no icw_ctx.
 */
#ifndef ICW_GRAPH_COMPILE_H
#define ICW_GRAPH_COMPILE_H

#include <string.h>

#include <vector>

#include "../../include/icw.h"
#include "icw_device.h"

#define ICW_PI_H (3.1415926535897932384626433832795029)

inline double u2d(unsigned long long u)
{
    double d;
    memcpy(&d, &u, 8);
    return d;
}

/* shared between the library's objects, not with its users: no dynamic symbols */
#pragma GCC visibility push(hidden)

unsigned fmt_size(unsigned fmt);
bool graph_accept(std::vector<icw_node> &n);
icw_node default_master();
int build_prog(const icw_config &cfg, std::vector<icw_node> nodes, IcwProg &P);
int build_prog_bus(const icw_config &cfg, std::vector<icw_node> nodes, IcwProg &P);
int icw_k4_cut_runs(const int32_t *ent, int count, std::vector<IcwK4Run> &runs, int *W);
void render_consts(const icw_render_cfg &cfg, int is24, bool spec, IcwRenderK &k);
bool needs_serial(const icw_config &cfg, const IcwRenderK &rk, const IcwProg &P, bool dith_par);
bool needs_render_state(const icw_config &cfg, const IcwRenderK &rk, const IcwProg &P, bool dith_par);
bool render_cfg_ok(const icw_render_cfg &r);
int plug_slot(const icw_node &n);
void matched_clears(const std::vector<icw_node> &o, const std::vector<icw_node> &nv, std::vector<int> &clears);

#pragma GCC visibility pop

#endif
