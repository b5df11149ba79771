// The one description of the SVGP calls' workspaces: gpx_svgp_prepare_f64, gpx_svgp_fit_collapsed_f64,
// gpx_svgp_bound_grad_f64, gpx_svgp_bound_grad_z_f64 and gpx_svgp_condition_f64.  svgp_layout walks every region once with a bump cursor; the reported sizes, the chunk width
// a given workspace allows (svgp_chunk_width) and the pointers the launches get (SvgpWorkspace) all come from it.  The
// fit is the gradient's layout without the gradient's regions, and the inducing-location gradient's is the gradient's
// plus two regions.  The conditioning call's is the fit's without the zero vector and the second info words (the
// task's alpha' and the caller's info take their places), plus the padded S of the preparation, which the compose step
// reads as its left operand.  gpx_svgp_acquire_f64's workspace is described at the end (svgp_acquire_layout).  No HIP in here:
// tests/host/svgp_layout_check.cpp
// compiles this file alone with the host compiler and checks it against a second statement of the layout.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gpx_sweep_layout.h"  // NB, up256

namespace gpx {

inline int64_t up128(int64_t v) { return (v + 127) / 128 * 128; }
// scratch of the triangular inverse and of the alpha product (gpx_trtri_workspace_size, gpx_alpha_workspace_size)
inline size_t trtri_ws(int64_t npad) { return (size_t)npad * npad / 4 * 8 + 256; }
inline size_t alpha_ws(int64_t npad, int64_t nrhs) { return ((size_t)(npad / 128) + 1) * npad * nrhs * 8 + 512; }
// the inverses of the factor's 64 x 64 diagonal blocks, twice (launch_potrf's Dinv)
inline size_t dinv_bytes(int64_t npad) { return (size_t)2 * (npad / NB) * NB * NB * 8; }

// The regions, in the order they lie in the workspace.  Per task: one block per task, `task` bytes apart, the offsets
// counted inside the block.  Shared: behind the last task's block, the offsets counted from the 256-aligned base.
enum SvgpRegion {
  // per task
  SV_A,      // Mpad x Mpad.  prepare: K_ZZ, then its factor L.  fit: K_ZZ, its factor, B_acc, B', L' (B' = L' L'^T);
             // gradient, between the passes: T1 = I - S, then G_A
  SV_WB,     // fit: Mpad x Mpad, W = L_ZZ^{-T}, then W' = L'^{-T}; gradient: then the products' intermediate U
  SV_DINV,   // the diagonal-block inverses (dinv_bytes)
  SV_SLICE,  // the triangular inverse's scratch; prepare: or the alpha product's, whichever is larger
  SV_SPAD,   // prepare, condition: Mpad x Mpad, S = tril(chol), zero-padded
  SV_MPAD,   // prepare: Mpad, m zero-padded
  SV_BVEC,   // fit: Mpad each: b', u, m' (reversed index order) ..
  SV_U,
  SV_MREV,
  SV_SCAL,   // .. and 256 bytes: the three scalar sums
  SV_WK,     // gradient: Mpad x Mpad each: W = L_ZZ^{-T}, kept
  SV_BC,     // B', then H
  SV_X1,     // Q
  SV_CV,     // Mpad each: c_v and m (natural order)
  SV_MNAT,
  SV_SC2,    // 512 bytes: the second pass's sums {sum e, e^T e, M - tr S, -, .., sum_i x_ik^2 at 8 + k}
  SV_GACC,   // the gradient accumulator row (nout doubles)
  SV_BND,    // 256 bytes: the bound's six values
  SV_ZACC,   // inducing-location gradient: the accumulator of dF/dZ, Mpad rows of zdim doubles
  // shared
  SV_ZERO,   // fit: Mpad zeros, standing in for the K* build's alpha
  SV_INFO2,  // ntask int32: the second factorisation's info words
  SV_KC,     // by chunk width: the covariance chunk, Mpad x ldk
  SV_PHI,    // one projected chunk per task, `phi_task` bytes apart (the tasks' rank updates share a launch)
  SV_MU,     // the K* build's mean partials, (Mpad / 64) x ldk
  SV_R,      // the chunk's residual, ldk
  SV_EV,     // gradient: the chunk's residual e, ldk
  SV_PART,   // the partial rows of one launch: (Mpad/128) max(Mpad/128, C/128) rows of nout doubles
  SV_ZPART,  // inducing-location gradient: one launch's row partials, (Mpad/128) (C/128) blocks of 128 x zdim doubles;
             // sized like SV_PART, for (Mpad/128) max(Mpad/128, C/128) blocks: two chunk widths whose gradient layouts
             // have one size then have one size here too, so a workspace sized for `chunk` by either gradient call's
             // size function gives both calls the same chunk width (and with it the same bits of `out`)
  SV_REGIONS,
  SV_SHARED = SV_ZERO  // the first shared region
};
enum SvgpKind { SVGP_PREPARE, SVGP_FIT, SVGP_GRAD, SVGP_GRAD_Z, SVGP_CONDITION };

struct SvgpLayout {
  struct Region { size_t at = 0, bytes = 0; };  // bytes = 0: not in this call's workspace
  Region r[SV_REGIONS];
  // what the driver clears with one memset: a span is exactly its members, contiguous and in order (the host check)
  Region acc;   // bvec, u, mrev, scal: the fit's vector accumulators and scalar sums
  Region acc2;  // sc2, gacc: the second pass's
  size_t task = 0;      // bytes between the tasks' blocks
  size_t phi_task = 0;  // bytes between the tasks' projected chunks
  int64_t ldk = 0;      // columns of the chunk-width regions: C rounded up to 256
  size_t total = 0;     // bytes from the aligned base; the reported size is total + 256
};

// Mpad: padded M; C: chunk width, a multiple of 128 (not used by prepare); nout: doubles of a gradient row
// (GPX_MLL_NOUT; the gradients only); zdim: doubles of a row of dF/dZ (GPX_MAX_DIM; SVGP_GRAD_Z only).
inline SvgpLayout svgp_layout(SvgpKind kind, int64_t Mpad, int64_t ntask, int64_t C = 0, int64_t nout = 0,
                              int64_t zdim = 0) {
  SvgpLayout L;
  const bool prep = kind == SVGP_PREPARE, fit = !prep, gz = kind == SVGP_GRAD_Z, grad = kind == SVGP_GRAD || gz;
  const bool cond = kind == SVGP_CONDITION;  // (the fit's regions but SV_ZERO and SV_INFO2, and SV_SPAD)
  const size_t mat = up256((size_t)Mpad * Mpad * 8), vec = up256((size_t)Mpad * 8);
  size_t at = 0;
  auto take = [&](SvgpRegion id, bool have, size_t bytes) {
    L.r[id].at = at;
    L.r[id].bytes = have ? bytes : 0;
    at += L.r[id].bytes;
  };
  auto span = [&](SvgpRegion first, SvgpRegion last) {
    return SvgpLayout::Region{L.r[first].at, L.r[last].at + L.r[last].bytes - L.r[first].at};
  };
  take(SV_A, true, mat);
  take(SV_WB, fit, mat);
  take(SV_DINV, true, up256(dinv_bytes(Mpad)));
  take(SV_SLICE, true, up256(prep && alpha_ws(Mpad, 1) > trtri_ws(Mpad) ? alpha_ws(Mpad, 1) : trtri_ws(Mpad)));
  take(SV_SPAD, prep || cond, mat);
  take(SV_MPAD, prep, vec);
  take(SV_BVEC, fit, vec);
  take(SV_U, fit, vec);
  take(SV_MREV, fit, vec);
  take(SV_SCAL, fit, 256);
  take(SV_WK, grad, mat);
  take(SV_BC, grad, mat);
  take(SV_X1, grad, mat);
  take(SV_CV, grad, vec);
  take(SV_MNAT, grad, vec);
  take(SV_SC2, grad, 512);
  take(SV_GACC, grad, up256((size_t)nout * 8));
  take(SV_BND, grad, 256);
  take(SV_ZACC, gz, up256((size_t)Mpad * zdim * 8));
  L.acc = span(SV_BVEC, SV_SCAL);
  L.acc2 = span(SV_SC2, SV_GACC);
  L.task = at;
  at = L.task * (size_t)ntask;
  L.ldk = (C + 255) / 256 * 256;
  L.phi_task = fit ? up256((size_t)Mpad * L.ldk * 8) : 0;
  const size_t nI = (size_t)(Mpad / 128), ncb = (size_t)(C / 128);
  take(SV_ZERO, fit && !cond, vec);
  take(SV_INFO2, fit && !cond, up256((size_t)ntask * 4));
  take(SV_KC, fit, L.phi_task);
  take(SV_PHI, fit, L.phi_task * (size_t)ntask);
  take(SV_MU, fit, up256((size_t)(Mpad / NB) * L.ldk * 8));
  take(SV_R, fit, up256((size_t)L.ldk * 8));
  take(SV_EV, grad, up256((size_t)L.ldk * 8));
  take(SV_PART, grad, up256(nI * (ncb > nI ? ncb : nI) * nout * 8));
  take(SV_ZPART, gz, up256(nI * (ncb > nI ? ncb : nI) * 128 * (size_t)zdim * 8));
  L.total = at;
  return L;
}

// The chunk width a workspace of ws_bytes allows the fit or the gradient: the largest multiple of 128, at most cap
// (GPX_SVGP_FIT_CHUNK) and the padded n, whose layout's reported size fits; 0 if none does.
inline int64_t svgp_chunk_width(SvgpKind kind, int64_t Mpad, int64_t ntask, int64_t n, int64_t cap, size_t ws_bytes,
                                int64_t nout = 0, int64_t zdim = 0) {
  int64_t C = cap < up128(n) ? cap : up128(n);
  while (C >= 128 && svgp_layout(kind, Mpad, ntask, C, nout, zdim).total + 256 > ws_bytes) C -= 128;
  return C >= 128 ? C : 0;
}

// Every pointer an SVGP call has into its workspace.  A region the layout leaves out (bytes = 0) is null.
struct SvgpWorkspace {
  SvgpLayout L;
  char* base;  // the caller's pointer rounded up to 256
  SvgpWorkspace(void* ws, const SvgpLayout& layout)
      : L(layout), base(reinterpret_cast<char*>(up256(reinterpret_cast<uintptr_t>(ws)))) {}
  template <class T = double>
  T* task(int64_t t, SvgpRegion id) const {
    return L.r[id].bytes && id < SV_SHARED ? reinterpret_cast<T*>(base + L.task * (size_t)t + L.r[id].at) : nullptr;
  }
  template <class T = double>
  T* shared(SvgpRegion id) const {
    return L.r[id].bytes && id >= SV_SHARED ? reinterpret_cast<T*>(base + L.r[id].at) : nullptr;
  }
  template <class T = double>
  T* task(int64_t t, const SvgpLayout::Region& span) const {  // (a clear span of the task's block)
    return span.bytes ? reinterpret_cast<T*>(base + L.task * (size_t)t + span.at) : nullptr;
  }
  int64_t pitch() const { return (int64_t)(L.task / sizeof(double)); }          // doubles between the tasks' blocks
  int64_t phi_pitch() const { return (int64_t)(L.phi_task / sizeof(double)); }  // and between their projected chunks
};

// gpx_svgp_acquire_f64's workspace: the sweep's (sweep_layout of the padded M and one right-hand side: the
// chunk's K*, the mean partials and the first product's variance partials, the block records the scoring launch
// writes; its pruned part is carried unused, so a buffer of this call's size serves gpx_svgp_predict_f64 too), and
// behind its total the call's own regions, each 256-aligned.  The offsets count from the same 256-aligned base as the
// sweep's, so none depends on the caller's pointer.  tests/host/svgp_acquire_layout_check.cpp checks it against a
// second statement.
enum SvgpAcquireRegion {
  SQ_SS2_PART,  // the second product's variance partials, (Mpad/128) x C doubles
  SQ_ACC_MU,    // the chunk's objective mean and variance over the tasks, C doubles each
  SQ_ACC_VAR,
  SQ_SCORES,    // the m scores where the caller passes scores_out = NULL
  SQ_SORT_WS,   // the selection's scratch (topk_workspace_bytes)
  SQ_REGIONS
};
struct SvgpAcquireLayout {
  SweepLayout sweep;  // SR_KSTAR, SR_MU_PART, SR_SS_PART, SR_REC_VAL, SR_REC_IDX are this call's
  SweepLayout::Region r[SQ_REGIONS];
  size_t total = 0;   // gpx_svgp_acquire_workspace_size
};
// sort_bytes: topk_workspace_bytes(m), which only the HIP side knows
inline SvgpAcquireLayout svgp_acquire_layout(int64_t Mpad, int64_t m, size_t sort_bytes) {
  SvgpAcquireLayout A;
  A.sweep = sweep_layout(Mpad, 1, m);
  size_t at = up256(A.sweep.total), reported = at + 256;  // (one more alignment step)
  auto take = [&](SvgpAcquireRegion id, size_t bytes) {
    A.r[id].at = at;
    A.r[id].bytes = bytes;
    at += bytes;
    reported += bytes;
  };
  take(SQ_SS2_PART, up256((size_t)(Mpad / TT) * A.sweep.C * 8));
  take(SQ_ACC_MU, up256((size_t)A.sweep.C * 8));
  take(SQ_ACC_VAR, up256((size_t)A.sweep.C * 8));
  take(SQ_SCORES, up256((size_t)m * 8));
  take(SQ_SORT_WS, up256(sort_bytes));
  A.total = reported;
  return A;
}

}  // namespace gpx
