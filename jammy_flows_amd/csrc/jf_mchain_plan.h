// Host-side plan of a chain of manifold layers ('r', 'o', 'm', 'f', 'v', 'c'): the rules a chain must pass and the layout of its parameter
// row, stated once for the five launchers that run such chains -- mchain (manifold_kernels.hip), mchain_bwd (manifold_bwd_kernels.hip),
// mchain_rev (manifold_rev_kernels.hip), grid_mchain (pair_kernels.hip) and cond_mchain (cond_manifold_kernels.hip).  Each of them calls
// plan_chain before it looks at the batch, so a chain is answered the same by every entry point and for every batch size, the empty one
// included; what only one launcher knows (its staging strides, its LDS formula, its grid) stays there and reads from the plan.
#pragma once
#include <type_traits>

#include "jf_expmap.h"
#include "jf_manifold.h"

namespace jf {

template <class Fam> struct ChainPlan {
    int n_layers;
    int P, max_row;                                    // the parameter row: its length, and the longest layer row
    int dim;                                           // columns of x the chain uses (<= Fam::DIM)
    int tab;                                           // per-lane elements of the widest knot table over the layers (0: no layer builds one)
    int corr;                                          // JF_CORR_SCRATCH if a layer is a correlated 'f', else 0
    int col0[JF_MAX_MCHAIN], ncols[JF_MAX_MCHAIN];     // every layer's first column and row length
};

// JF_OK, or why no kernel runs this chain: JF_ERR_UNSUPPORTED for options beyond the kernels, JF_ERR_BADARG for a descriptor that makes no sense
template <class Fam> __host__ int plan_chain(const typename Fam::CLayer* layers, int n_layers, ChainPlan<Fam>& p) {
    if (!layers || n_layers < 1 || n_layers > JF_MAX_MCHAIN) return JF_ERR_BADARG;
    for (int l = 0; l < n_layers; ++l) {               // (sane before any row-length arithmetic: jf_manifold.h)
        if (!Fam::supported(layers[l])) return JF_ERR_UNSUPPORTED;
        if (!Fam::sane(layers[l])) return JF_ERR_BADARG;
    }
    p = ChainPlan<Fam>{};
    p.n_layers = n_layers;
    p.dim = Fam::DIM;
    if constexpr (std::is_same<Fam, CFam>::value) {    // one kind per chain: it decides the columns of x
        for (int l = 1; l < n_layers; ++l) if (layers[l].kind != layers[0].kind) return JF_ERR_BADARG;
        p.dim = layers[0].kind == 2 ? 2 : 1;
    }
    for (int l = 0; l < n_layers; ++l) {
        const int n = Fam::row_len(layers[l]);
        p.col0[l] = p.P; p.ncols[l] = n;
        p.P += n;
        if (n > p.max_row) p.max_row = n;
        if (Fam::needs_tab(layers[l])) { const int w = fam_tab_words<Fam>::of(layers[l]); p.tab = w > p.tab ? w : p.tab; }
    }
    if constexpr (std::is_same<Fam, FFam>::value) {    // the correlated MLP's emitted parameters + rank accumulators live in the lane's scratch
        for (int l = 0; l < n_layers; ++l) {
            if (!layers[l].correlated) continue;
            if (layers[l].corr_hidden < 1 || layers[l].corr_rank < 0 || FFam::corr_out(layers[l]) + layers[l].corr_rank > JF_CORR_SCRATCH - 1)
                return JF_ERR_UNSUPPORTED;
            p.corr = JF_CORR_SCRATCH;
        }
    }
    return JF_OK;
}

}  // namespace jf
