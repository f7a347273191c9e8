// The satellite units' context state (vba_sat.hpp) as the BA core sees it: made with the context, released with it.  Host code only:
// this unit compiles no kernel header, so that a new satellite field rebuilds its owner and these few lines.
#include "vba_ctx.hpp"
#include "vba_sat.hpp"

#include <new>

namespace vba {

int ctx_sat_create(vba_ctx *c) {
  c->sat = new (std::nothrow) CtxSat();
  return c->sat ? VBA_OK : VBA_ERR_CAPACITY;
}

void ctx_sat_release(vba_ctx *c) {
  delete c->sat;
  c->sat = nullptr;
}

}  // namespace vba
