// capi_internal.hpp -- what other library components (the native Krylov solver, krylov.cpp) may see of a hymls_mi
// handle.  Defined in capi.cpp; not part of the public C ABI.
#pragma once
#include "../../include/hymls_mi.h"
#include "precond.hpp"

namespace hymls {

struct HandleView {
  LevelSolver* top = nullptr;     // the level-0 solver (nullptr before Initialize)
  const Comm* comm = nullptr;     // the handle's communicator (one rank unless set)
  dev::Context* ctx = nullptr;    // bind it before touching the device
  bool computed = false;
  std::string* err = nullptr;     // the handle's last-error text
};
HandleView handle_view(hymls_mi_t* h);

}  // namespace hymls
