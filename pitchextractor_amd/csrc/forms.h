// Where a request at the C ABI -- `int products` (pe_products) and `int act16` -- becomes a kernel instance.  Every
// entry point that takes one of the two goes through with_form / with_act; nothing else switches on them.
#pragma once
#include "gemm_engine.h"

namespace pe {

// One product form: the tile engines' MODE (terms per operand: mode_terms<MODE>()), the activation tensors' element
// type TA and the 16-bit type TH that one-term operands are rounded to.
template <int MODE_, class TA_ = float, class TH_ = __bf16>
struct Form {
  static constexpr int MODE = MODE_;
  typedef TA_ TA;
  typedef TH_ TH;
};

constexpr unsigned form_bit(int products) { return 1u << products; }
constexpr unsigned kAllForms = form_bit(PE_PROD_F16 + 1) - 1;
constexpr unsigned kTermForms = kAllForms & ~form_bit(PE_PROD_NATIVE);   // forms made of 16-bit terms

// Calls fn(Form<...>{}) with the form that (products, act16) selects and returns its status.  SERVED: mask of the
// pe_products values the caller has kernels for; ACT16: whether it has the bf16-activation instance, which exists under
// PE_PROD_BF16 only.  Anything else is pe_unserved(products), and fn is not instantiated for it.
template <unsigned SERVED, bool ACT16, class Fn>
int with_form(int products, int act16, Fn&& fn) {
  static_assert(!ACT16 || (SERVED & form_bit(PE_PROD_BF16)), "bf16 activations come with the bf16 form");
  if (act16) {
    if constexpr (ACT16)
      if (products == PE_PROD_BF16) return fn(Form<kBf16, act16_t>{});
    return pe_unserved(products);
  }
  if constexpr ((SERVED & form_bit(PE_PROD_NATIVE)) != 0)
    if (products == PE_PROD_NATIVE) return fn(Form<kNative>{});
  if constexpr ((SERVED & form_bit(PE_PROD_X3)) != 0)
    if (products == PE_PROD_X3) return fn(Form<kSplit>{});
  if constexpr ((SERVED & form_bit(PE_PROD_H2)) != 0)
    if (products == PE_PROD_H2) return fn(Form<kSplit2>{});
  if constexpr ((SERVED & form_bit(PE_PROD_BF16)) != 0)
    if (products == PE_PROD_BF16) return fn(Form<kBf16>{});
  if constexpr ((SERVED & form_bit(PE_PROD_F16)) != 0)
    if (products == PE_PROD_F16) return fn(Form<kBf16, float, _Float16>{});
  return pe_unserved(products);
}

// The entry points that take `act16` alone: fn(ActType<float>{}) or fn(ActType<act16_t>{}).
template <class T> struct ActType { typedef T TA; };
template <class Fn>
int with_act(int act16, Fn&& fn) {
  return act16 ? fn(ActType<act16_t>{}) : fn(ActType<float>{});
}

}  // namespace pe
