// oracle/cvstub/glog/logging.h  --  TEST INFRASTRUCTURE ONLY (see ../opencv2/core.hpp).
// CHECK_EQ and LOG(FATAL) as the reference uses them: a failed check or a fatal message prints to stderr and aborts.
#ifndef CVSTUB_GLOG_LOGGING_H
#define CVSTUB_GLOG_LOGGING_H
#include <cstdlib>
#include <iostream>
namespace cvstub_log {
struct Fatal {
  Fatal(const char* file, int line, const char* what) { std::cerr << file << ":" << line << ": " << what << " "; }
  template <typename T> Fatal& operator<<(const T& v) { std::cerr << v; return *this; }
  [[noreturn]] ~Fatal() { std::cerr << std::endl; std::abort(); }
};
struct Voidify { void operator&(const Fatal&) {} };
}
#define LOG(severity) cvstub_log::Fatal(__FILE__, __LINE__, "LOG(" #severity ")")
#define CHECK_EQ(a, b) ((a) == (b)) ? (void)0 : cvstub_log::Voidify() & cvstub_log::Fatal(__FILE__, __LINE__, "CHECK_EQ(" #a ", " #b ") failed")
#endif
