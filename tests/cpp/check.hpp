// What every test program of this directory shares: the two counters, the CHECK macros, near() and the closing summary line.
// A program includes this header, runs its CHECKs and ends with `return finish("test_name");` -- the line "<n> checks, <k> failed"
// is what tests/cpp_programs.py looks for.
#pragma once
#include <cmath>
#include <cstdio>

inline int g_checks = 0, g_failed = 0;

#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
// the same with a printf-style message instead of the condition's text
#define CHECKF(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)
// expr throws an Error (include/relp.hpp; the name is looked up where the macro is used) whose status() is `code`
#define CHECK_THROWS(expr, code)                                                                      \
    do {                                                                                              \
        ++g_checks;                                                                                   \
        bool thrown_ = false;                                                                         \
        try { (void)(expr); } catch (const Error& e) { thrown_ = e.status() == (code); }              \
        if (!thrown_) { ++g_failed; std::printf("FAILED %s:%d: %s did not throw %s\n", __FILE__, __LINE__, #expr, #code); } \
    } while (0)

// |a - b| <= tol max(1, |b|); every program states its own tolerance
inline bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol * std::fmax(1.0, std::fabs(b)); }

// the summary line and the exit code of main
inline int finish(const char* name) {
    std::printf("%s: %d checks, %d failed\n", name, g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
