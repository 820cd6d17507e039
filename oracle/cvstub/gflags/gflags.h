// oracle/cvstub/gflags/gflags.h  --  TEST INFRASTRUCTURE ONLY (see ../opencv2/core.hpp).
// The reference's util.hpp declares two flags of the flag library's namespace as extern; they are defined here (weak, so every
// translation unit may carry the definition) and read by nothing that is compiled against the stand-in.
#ifndef CVSTUB_GFLAGS_H
#define CVSTUB_GFLAGS_H
namespace fLB {
__attribute__((weak)) bool FLAGS_help = false;
__attribute__((weak)) bool FLAGS_helpshort = false;
}
#endif
