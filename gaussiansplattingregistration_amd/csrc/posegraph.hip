// posegraph.hip -- gsr_posegraph_optimize (include/gsr_hip.h): the C entry of the pose-graph optimiser in gsr_posegraph.h.  Host code
// only, like gsr_icp_solve: no device is touched, and it works on a machine without one.
#include "gsr_common.h"
#include "gsr_posegraph.h"

using namespace gsr;

extern "C" int32_t gsr_posegraph_optimize(int32_t n_nodes, double* poses, int32_t n_edges, const gsr_pose_edge* edges, const gsr_posegraph_option* option,
                                          double* line_process, int32_t* pruned, gsr_posegraph_result* result) {
    if (n_nodes < 1 || !poses) return fail(GSR_E_INVALID, "gsr_posegraph_optimize: no nodes (n_nodes %d)", n_nodes);
    if (n_edges < 0 || (n_edges > 0 && !edges)) return fail(GSR_E_INVALID, "gsr_posegraph_optimize: %d edges and no edge array", n_edges);
    posegraph::Option o;
    if (option) {
        o.max_correspondence_distance = option->max_correspondence_distance;
        o.edge_prune_threshold = option->edge_prune_threshold;
        o.preference_loop_closure = option->preference_loop_closure;
        o.reference_node = option->reference_node;
        o.max_iteration = option->max_iteration;
        o.max_iteration_lm = option->max_iteration_lm;
        o.min_relative_increment = option->min_relative_increment;
        o.min_relative_residual_increment = option->min_relative_residual_increment;
        o.min_right_term = option->min_right_term;
        o.min_residual = option->min_residual;
    }
    std::vector<posegraph::Edge> E((size_t)n_edges);
    for (int k = 0; k < n_edges; ++k) {
        E[k].s = edges[k].source;
        E[k].t = edges[k].target;
        E[k].uncertain = edges[k].uncertain != 0;
        memcpy(E[k].T, edges[k].T, sizeof E[k].T);
        memcpy(E[k].info, edges[k].information, sizeof E[k].info);
    }
    posegraph::Result r;
    const std::string err = posegraph::optimize(n_nodes, poses, E, o, line_process, pruned, &r);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_posegraph_optimize: %s", err.c_str());
    if (result) {
        result->iterations[0] = r.iterations[0];
        result->iterations[1] = r.iterations[1];
        result->n_pruned = r.n_pruned;
        result->reserved = 0;
        result->E_initial = r.E_initial;
        result->E_final = r.E_final;
        result->mu = r.mu;
        result->mu_first = r.mu_first;
    }
    return GSR_OK;
}
