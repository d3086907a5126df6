// CPU ORACLE — TEST INFRASTRUCTURE ONLY.
// C entry points over the REFERENCE's own number-string comparators, compiled from the header where it lies
// (/root/reference/src/util/string.h: util::StringNumCmp, <string> only); nothing of the reference is copied into
// this repo. Built only in the authoring container (oracle/build_oracle.py -> oracle/_ref/libviya_numcmp.so) and used
// to (1) validate oracle/viya_oracle.py's _cmp_strings restatement and (2) generate tests/golden/numcmp_golden.json
// (oracle/make_numcmp_golden.py). Each returns 1 / 0, or -1 where std::stod threw.
#include "util/string.h"

namespace vu = viya::util;

template <typename F> static int guarded(F f) {
  try {
    return f() ? 1 : 0;
  } catch (...) {
    return -1;
  }
}

extern "C" {
int ref_greater_int(const char* a, const char* b) { return guarded([&] { return vu::StringNumCmp::GreaterInt(a, b); }); }
int ref_smaller_int(const char* a, const char* b) { return guarded([&] { return vu::StringNumCmp::SmallerInt(a, b); }); }
int ref_greater_float(const char* a, const char* b) { return guarded([&] { return vu::StringNumCmp::GreaterFloat(a, b); }); }
int ref_smaller_float(const char* a, const char* b) { return guarded([&] { return vu::StringNumCmp::SmallerFloat(a, b); }); }
}
