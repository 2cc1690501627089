// The block forms every tiled kernel family is instantiated for, and the dispatchers that turn a run-time form into
// a compile-time one.  Host-only (no HIP types), like host_plan.hpp, which includes it.
//
// A form is M rows per element and CMP, compressed or dense couplings; the chain and cyclic-reduction families know
// M alone; the K-column families add a column group KB.  Each family has ONE predicate here.  The level predicates and
// the tile planners ask it, and the launchers go through with_form / with_block_size, whose `if constexpr` guard
// instantiates exactly the forms the predicate names: a predicate and a dispatcher cannot disagree.
#pragma once
#include <type_traits>
#include <utility>

namespace aggmg {

constexpr int kMaxBlock = 9;   // rows per element: no family is instantiated beyond

// ---- the lists ---------------------------------------------------------------------------------------------------
// the fused block-tridiagonal kernel (btd_fused_kernel): every element-block form set-up produces
constexpr bool btd_form(int m, bool cmp) { return cmp ? (m >= 2 && m <= 9) : (m >= 1 && m <= 5); }
// ... of those, the forms with the symmetric packing of B^{-1} and the couplings
constexpr bool btd_sym_form(int m, bool cmp) { return cmp ? (m == 2 || m == 4 || m == 8) : (m == 2 || m == 4); }
// ... and of those, the forms of the lossless symmetric residual, the operator dictionary and the element-thread kernels
constexpr bool btd_sres_form(int m, bool cmp) { return cmp && m <= 4 && btd_sym_form(m, cmp); }
// the element-patch sweep kernels (patch_sweep_kernel, patch_gs_kernel, patch_gs_up_kernel): up to 8 rows per element
constexpr bool patch_form(int m, bool cmp) { return m <= 8 && btd_form(m, cmp); }
// the K-column kernels (btd_multi_kernel, btd_residual_multi_kernel, patch_gs_multi_kernel)
constexpr bool multi_form(int m, bool cmp) { return cmp ? (m == 2 || m == 4) : m == 2; }
constexpr bool multi_block_size(int m) { return multi_form(m, true) || multi_form(m, false); }   // ... their lane groups
// the chain kernel (cgt_fused_kernel), and its dictionary and K-column variants (lane groups of m)
constexpr bool chain_form(int m) { return m >= 1 && m <= 8; }
constexpr bool chain_dict_form(int m) { return m == 1 || m == 2 || m == 4; }
// the cyclic reduction of the coarsest solve; the block inversion of set-up (larger blocks take its any-size kernel)
constexpr bool cr_form(int m) { return m >= 1 && m <= 8; }
constexpr bool invert_form(int m) { return m >= 1 && m <= 8; }
// ... its chunk stages with the factor records in LDS (cr_stage_forward_dict_kernel, cr_stage_backward_dict_kernel): the
// block sizes whose sub-chunk factors are fetched in one batch
constexpr bool cr_dict_form(int m) { return m == 1 || m == 2; }
// lanes per row of csr_row_kernel
constexpr bool csr_lanes_form(int l) { return l >= 1 && l <= 64 && (l & (l - 1)) == 0; }

// The smallest instantiated column group (1, 2, 4, 8) that holds kc columns.  ceiling: the cycle's group where it is
// smaller than 8 -- the larger groups are never chosen then.
constexpr int col_group(int kc, int ceiling = 8) {
  return kc <= 1 ? 1 : (kc <= 2 || ceiling == 2) ? 2 : (kc <= 4 || ceiling == 4) ? 4 : 8;
}
constexpr bool is_col_group(int kb) { return kb >= 1 && kb <= 8 && col_group(kb) == kb; }

// ---- the dispatchers ---------------------------------------------------------------------------------------------
template <int M, bool CMP>
struct Form {
  static constexpr int kM = M;
  static constexpr bool kCmp = CMP;
};

// f(std::integral_constant<int, M>{}) for the M in 1 .. Max with Pred(M) that equals m; false when there is none
template <auto Pred, int M, class F>
bool with_block_size_at(int m, F& f) {
  if constexpr (Pred(M)) {
    if (m == M) {
      f(std::integral_constant<int, M>{});
      return true;
    }
  }
  return false;
}
// (from the largest size down: the kernels then stand in a translation unit's code object in the order the switch
// statements before this header left them in, and a build-to-build comparison of the code objects shows no change)
template <auto Pred, class F, int... I>
bool with_block_size_in(int m, F& f, std::integer_sequence<int, I...>) {
  return (with_block_size_at<Pred, (int)sizeof...(I) - I>(m, f) || ...);
}
template <auto Pred, int Max = kMaxBlock, class F>
bool with_block_size(int m, F&& f) {
  return with_block_size_in<Pred>(m, f, std::make_integer_sequence<int, Max>{});
}

// f(Form<M, CMP>{}) for the form with Pred(M, CMP) that equals (m, cmp); false when there is none
template <auto Pred, int M, bool CMP, class F>
bool with_form_at(int m, bool cmp, F& f) {
  if constexpr (Pred(M, CMP)) {
    if (m == M && cmp == CMP) {
      f(Form<M, CMP>{});
      return true;
    }
  }
  return false;
}
template <auto Pred, class F, int... I>
bool with_form_in(int m, bool cmp, F& f, std::integer_sequence<int, I...>) {
  return ((with_form_at<Pred, I + 1, true>(m, cmp, f) || with_form_at<Pred, I + 1, false>(m, cmp, f)) || ...);
}
template <auto Pred, class F>
bool with_form(int m, bool cmp, F&& f) {
  return with_form_in<Pred>(m, cmp, f, std::make_integer_sequence<int, kMaxBlock>{});
}

// f(std::integral_constant<int, KB>{}) for KB = col_group(kc, ceiling)
template <class F>
void with_col_group(int kc, int ceiling, F&& f) {
  with_block_size<is_col_group, 8>(col_group(kc, ceiling), f);
}
template <class F>
void with_col_group(int kc, F&& f) {
  with_col_group(kc, 8, f);
}

// ---- the lists are today's: bit m of a mask is block size m -----------------------------------------------------------
constexpr unsigned form_mask(bool (*pred)(int, bool), bool cmp) {
  unsigned s = 0;
  for (int m = 0; m < 32; ++m) s |= pred(m, cmp) ? 1u << m : 0u;
  return s;
}
constexpr unsigned size_mask(bool (*pred)(int)) {
  unsigned s = 0;
  for (int m = 0; m < 32; ++m) s |= pred(m) ? 1u << m : 0u;
  return s;
}
constexpr int count_bits(unsigned s) { return s ? (int)(s & 1u) + count_bits(s >> 1) : 0; }
constexpr int count_forms(bool (*pred)(int, bool)) { return count_bits(form_mask(pred, true)) + count_bits(form_mask(pred, false)); }

static_assert(form_mask(btd_form, true) == 0b1111111100 && form_mask(btd_form, false) == 0b111110 && count_forms(btd_form) == 13,
              "btd_form: compressed 2..9 and dense 1..5");
static_assert(form_mask(btd_sym_form, true) == 0b100010100 && form_mask(btd_sym_form, false) == 0b10100, "btd_sym_form: compressed 2, 4, 8; dense 2, 4");
static_assert(form_mask(btd_sres_form, true) == 0b10100 && form_mask(btd_sres_form, false) == 0, "btd_sres_form: compressed 2, 4");
static_assert(form_mask(patch_form, true) == 0b111111100 && form_mask(patch_form, false) == 0b111110 && count_forms(patch_form) == 12,
              "patch_form: compressed 2..8 and dense 1..5");
static_assert(form_mask(multi_form, true) == 0b10100 && form_mask(multi_form, false) == 0b100 && count_forms(multi_form) == 3,
              "multi_form: compressed 2, 4; dense 2");
static_assert(size_mask(multi_block_size) == 0b10100, "the K-column lane groups: 2, 4");
static_assert(size_mask(chain_form) == 0b111111110 && size_mask(cr_form) == 0b111111110 && size_mask(invert_form) == 0b111111110,
              "chain_form, cr_form, invert_form: 1..8");
static_assert(size_mask(chain_dict_form) == 0b10110 && count_bits(size_mask(chain_dict_form)) == 3, "chain_dict_form: 1, 2, 4");
static_assert(size_mask(cr_dict_form) == 0b110, "cr_dict_form: 1, 2");
static_assert(size_mask(is_col_group) == 0b100010110, "column groups: 1, 2, 4, 8");
static_assert(col_group(1) == 1 && col_group(2) == 2 && col_group(3) == 4 && col_group(4) == 4 && col_group(5) == 8 && col_group(8) == 8 &&
                  col_group(3, 2) == 2 && col_group(8, 4) == 4 && col_group(3, 4) == 4,
              "col_group: the smallest of 1, 2, 4, 8 that holds kc, never above a ceiling of 2 or 4");

}  // namespace aggmg
