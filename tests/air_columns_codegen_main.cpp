// The source text csrc/air_codegen.h writes for a columns (STORE) program (tests/test_cpu_air_columns_codegen.py): the twin of
// tests/air_codegen_main.cpp.  Every input line is "n_cols n_out w0 w1 w0 w1 ..." (decimal words); the answer to a line is
// "error: <reason>" or "ok <bytes>" followed by that many bytes of source text and a newline.  With an argument "compile" (and
// built with -DAIR_CODEGEN_HIPRTC, linked against hipRTC) each accepted text is also compiled for gfx950 with the option list of
// the header (no device is needed), and "ok" becomes "ok <bytes> <code object bytes> <compile milliseconds>" and then, for
// air_columns_w4 and for air_columns_w1, the VGPRs, SGPRs and private-segment bytes the code object's metadata states
// (code_object_uint of the header; -1 where it finds none); a failed compilation is "error: hiprtc: <log>".
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "air_codegen.h"

#ifdef AIR_CODEGEN_HIPRTC
#include <hip/hiprtc.h>

static bool compile(const std::string &src, std::vector<char> &code, std::string &log) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "air_columns.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return false;
    }
    std::vector<const char *> opts = {"--offload-arch=gfx950"};
    for (const char *o : tstwo::kAirNativeOptions) opts.push_back(o);
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t n = 0;
    if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        log.resize(n);
        hiprtcGetProgramLog(prog, &log[0]);
    }
    size_t code_bytes = 0;
    bool ok = rc == HIPRTC_SUCCESS && hiprtcGetCodeSize(prog, &code_bytes) == HIPRTC_SUCCESS && code_bytes > 0;
    if (ok) {
        code.resize(code_bytes);
        ok = hiprtcGetCode(prog, code.data()) == HIPRTC_SUCCESS;
    }
    hiprtcDestroyProgram(&prog);
    return ok;
}
#endif

int main(int argc, char **argv) {
    const bool want_compile = argc > 1 && !std::strcmp(argv[1], "compile");
#ifndef AIR_CODEGEN_HIPRTC
    if (want_compile) {
        std::fprintf(stderr, "built without hipRTC\n");
        return 2;
    }
#endif
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        size_t n_cols, n_out;
        if (!(in >> n_cols >> n_out)) continue;
        std::vector<uint32_t> words;
        uint64_t w;
        while (in >> w) words.push_back((uint32_t)w);
        std::string src;
        if (const char *why = tstwo::air_columns_codegen(words.data(), words.size() / 2, n_cols, n_out, src)) {
            std::printf("error: %s\n", why);
            continue;
        }
        if (want_compile) {
#ifdef AIR_CODEGEN_HIPRTC
            std::vector<char> code;
            std::string log;
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = compile(src, code, log);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) {
                for (char &c : log) if (c == '\n') c = ' ';
                std::printf("error: hiprtc: %s\n", log.c_str());
                continue;
            }
            std::printf("ok %zu %zu %.0f", src.size(), code.size(), ms);
            for (const char *kernel : {tstwo::kAirColumnsKernelW4, tstwo::kAirColumnsKernelW1})
                for (const char *key : {".vgpr_count", ".sgpr_count", ".private_segment_fixed_size"}) {
                    uint32_t v = 0;
                    if (tstwo::code_object_uint(code.data(), code.size(), kernel, key, v)) std::printf(" %u", v);
                    else std::printf(" -1");
                }
            std::printf("\n");
#endif
        } else {
            std::printf("ok %zu\n", src.size());
        }
        std::fwrite(src.data(), 1, src.size(), stdout);
        std::printf("\n");
    }
    return 0;
}
