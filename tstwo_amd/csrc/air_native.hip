// air_native.hip — constraint programs compiled to gfx950 kernels at run time (the opt-in twin of the interpreter k_air_program).
// tstwo_air_program_compile turns a program into HIP source (csrc/air_codegen.h: straight-line code on local variables, no LDS
// register file, so the compiler keeps many column loads in flight), compiles it with hipRTC for the architecture of the current
// device and loads the code object; tstwo_air_eval_compiled (air.hip) checks its arguments as tstwo_air_eval_program does and
// launches it here.  A kernel is named by an id into the table below, never by a pointer: ids are handed out once and are not
// reused, so a destroyed id, or one from before tstwo_shutdown, is simply not found.  tstwo_air_columns_compile does the same for
// the STORE programs of tstwo_air_eval_columns (air_columns_codegen; tstwo_air_eval_columns_compiled launches them): one table, one
// id counter, and every entry knows which of the two kinds it is.
//
// hipRTC is bound at first use (dlopen / dlsym, as comm.hip binds RCCL), not at link time: it brings the whole compiler
// (libamd_comgr) into the process, which a prover that never compiles should not pay for at load, and a process that already
// holds a copy shares it.  The library is looked for by name and beside the HIP runtime this library itself runs on.
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <chrono>
#include <unordered_map>
#include <vector>

#include "air_codegen.h"
#include "air_native.h"

using namespace tstwo;

namespace {

struct Hiprtc {
    void *handle = nullptr;
    decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
    decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
    decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
    decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
    decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
    decltype(&hiprtcGetCode) GetCode = nullptr;
    decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
    decltype(&hiprtcGetErrorString) GetErrorString = nullptr;
};
Hiprtc g_rtc;

int load_hiprtc() {
    if (g_rtc.handle) return TSTWO_OK;
    std::vector<std::string> names = {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6"};
    Dl_info runtime;                         // beside the HIP runtime in use
    if (dladdr((void *)&hipModuleLoadData, &runtime) && runtime.dli_fname) {
        const std::string path(runtime.dli_fname);
        const size_t slash = path.rfind('/');
        if (slash != std::string::npos) names.push_back(path.substr(0, slash + 1) + "libhiprtc.so");
    }
    void *h = nullptr;
    for (const std::string &n : names)       // a copy already mapped by the process first
        if (!h) h = dlopen(n.c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);
    for (const std::string &n : names)
        if (!h) h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        const char *e = dlerror();
        return set_error(TSTWO_ERR_HIP, std::string("hipRTC is not available: ") + (e ? e : "libhiprtc.so not found"));
    }
    Hiprtc r;
    r.handle = h;
    r.CreateProgram = (decltype(r.CreateProgram))dlsym(h, "hiprtcCreateProgram");
    r.CompileProgram = (decltype(r.CompileProgram))dlsym(h, "hiprtcCompileProgram");
    r.DestroyProgram = (decltype(r.DestroyProgram))dlsym(h, "hiprtcDestroyProgram");
    r.GetProgramLog = (decltype(r.GetProgramLog))dlsym(h, "hiprtcGetProgramLog");
    r.GetProgramLogSize = (decltype(r.GetProgramLogSize))dlsym(h, "hiprtcGetProgramLogSize");
    r.GetCode = (decltype(r.GetCode))dlsym(h, "hiprtcGetCode");
    r.GetCodeSize = (decltype(r.GetCodeSize))dlsym(h, "hiprtcGetCodeSize");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "hiprtcGetErrorString");
    if (!r.CreateProgram || !r.CompileProgram || !r.DestroyProgram || !r.GetProgramLog || !r.GetProgramLogSize || !r.GetCode ||
        !r.GetCodeSize || !r.GetErrorString)
        return set_error(TSTWO_ERR_HIP, "the hipRTC library lacks hiprtcCreateProgram / hiprtcCompileProgram / hiprtcGetCode");
    g_rtc = r;
    return TSTWO_OK;
}

struct Kernel {
    hipModule_t module = nullptr;
    hipFunction_t fn[2] = {nullptr, nullptr};        // W = 4, W = 1
    AirKernelKind kind = kAirKernelConstraints;
    u32 n_cols = 0, n_terminal = 0;                  // n_terminal: the constraints (ACC) or the outputs (STORE) it was compiled for
    u32 sgprs[2] = {0, 0};                           // from the code object's metadata (the runtime does not report them)
    size_t code_bytes = 0;
};
std::unordered_map<uint64_t, Kernel> g_kernels;
uint64_t g_next_id = 1;                              // never reset: an id is handed out once per process

int bad(const std::string &msg) { return set_error(TSTWO_ERR_BAD_ARG, msg); }

Kernel *find(uint64_t id) {
    auto it = g_kernels.find(id);
    return it == g_kernels.end() ? nullptr : &it->second;
}

// source text -> code object for `arch`; on failure the compiler's log is the error text
int compile(const std::string &src, const std::string &arch, std::vector<char> &code) {
    if (int rc = load_hiprtc()) return rc;
    hiprtcProgram prog = nullptr;
    hiprtcResult r = g_rtc.CreateProgram(&prog, src.c_str(), "air_native.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) return set_error(TSTWO_ERR_HIP, std::string("air program compile: hiprtcCreateProgram: ") + g_rtc.GetErrorString(r));
    const std::string arch_opt = "--offload-arch=" + arch;
    std::vector<const char *> opts = {arch_opt.c_str()};
    for (const char *o : kAirNativeOptions) opts.push_back(o);
    r = g_rtc.CompileProgram(prog, (int)opts.size(), opts.data());
    int rc = TSTWO_OK;
    size_t n = 0;
    if (r != HIPRTC_SUCCESS) {
        std::string log;
        if (g_rtc.GetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            (void)g_rtc.GetProgramLog(prog, &log[0]);
        }
        rc = set_error(TSTWO_ERR_HIP, std::string("air program compile: ") + g_rtc.GetErrorString(r) + ": " + log.c_str());
    } else if ((r = g_rtc.GetCodeSize(prog, &n)) != HIPRTC_SUCCESS || n == 0) {
        rc = set_error(TSTWO_ERR_HIP, std::string("air program compile: hiprtcGetCodeSize: ") + g_rtc.GetErrorString(r));
    } else {
        code.resize(n);
        if ((r = g_rtc.GetCode(prog, code.data())) != HIPRTC_SUCCESS)
            rc = set_error(TSTWO_ERR_HIP, std::string("air program compile: hiprtcGetCode: ") + g_rtc.GetErrorString(r));
    }
    (void)g_rtc.DestroyProgram(&prog);
    return rc;
}

const char *kernel_name(AirKernelKind kind, int w) {
    return kind == kAirKernelColumns ? (w == 0 ? kAirColumnsKernelW4 : kAirColumnsKernelW1) : (w == 0 ? kAirNativeKernelW4 : kAirNativeKernelW1);
}

// compiles `src` for the current device, loads it and enters its two kernels into the table under a fresh id
int compile_and_register(const std::string &src, AirKernelKind kind, size_t n_cols, size_t n_terminal, uint64_t *kernel_id) {
    hipDeviceProp_t prop;
    TSTWO_HIP(hipGetDeviceProperties(&prop, ctx().device));
    std::vector<char> code;
    if (int rc = compile(src, prop.gcnArchName, code)) return rc;
    Kernel k;
    k.kind = kind;
    k.n_cols = (u32)n_cols;
    k.n_terminal = (u32)n_terminal;
    k.code_bytes = code.size();
    TSTWO_HIP(hipModuleLoadData(&k.module, code.data()));
    for (int w = 0; w < 2; w++) {
        const hipError_t e = hipModuleGetFunction(&k.fn[w], k.module, kernel_name(kind, w));
        if (e != hipSuccess) {
            (void)hipModuleUnload(k.module);
            return hip_fail(e, "hipModuleGetFunction");
        }
        (void)code_object_uint(code.data(), code.size(), kernel_name(kind, w), ".sgpr_count", k.sgprs[w]);
    }
    *kernel_id = g_next_id++;
    g_kernels[*kernel_id] = k;
    return TSTWO_OK;
}

}  // namespace

namespace tstwo {

int air_native_shape(uint64_t id, AirKernelKind &kind, u32 &n_cols, u32 &n_terminal) {
    const Kernel *k = find(id);
    if (!k) return bad("unknown air kernel");
    kind = k->kind;
    n_cols = k->n_cols;
    n_terminal = k->n_terminal;
    return TSTWO_OK;
}

int air_native_launch(uint64_t id, const AirPlan &plan, ColPtrs &cols, NativeArgs &args) {
    const Kernel *k = find(id);
    if (!k || k->kind != kAirKernelConstraints) return bad("unknown air kernel");
    args.stride = plan.stride;
    void *params[] = {&cols, &args};
    TSTWO_HIP(hipModuleLaunchKernel(k->fn[plan.w == 4 ? 0 : 1], plan.grid, 1, 1, plan.threads, 1, 1, 0, ctx().stream, params, nullptr));
    return TSTWO_OK;
}

int air_native_launch_columns(uint64_t id, const AirPlan &plan, ColPtrs &cols, ColPtrs &out, ColumnsArgs &args) {
    const Kernel *k = find(id);
    if (!k || k->kind != kAirKernelColumns) return bad("unknown air kernel");
    args.stride = plan.stride;
    void *params[] = {&cols, &out, &args};
    TSTWO_HIP(hipModuleLaunchKernel(k->fn[plan.w == 4 ? 0 : 1], plan.grid, 1, 1, plan.threads, 1, 1, 0, ctx().stream, params, nullptr));
    return TSTWO_OK;
}

void air_native_shutdown() {
    for (auto &kv : g_kernels) (void)hipModuleUnload(kv.second.module);
    g_kernels.clear();
}

}  // namespace tstwo

extern "C" {

int tstwo_air_program_compile(const u32 *program, size_t program_len, size_t n_cols, size_t n_constraints, uint64_t *kernel_id) {
    TSTWO_REQUIRE_READY();
    if (!program || !kernel_id) return bad("null host argument");
    if (stream_is_capturing()) return bad("air program compile: refused during graph capture (it loads a module, synchronously)");
    std::string src;
    if (const char *why = air_codegen(program, program_len, n_cols, n_constraints, src)) return bad(std::string("air program: ") + why);
    return compile_and_register(src, kAirKernelConstraints, n_cols, n_constraints, kernel_id);
}

int tstwo_air_columns_compile(const u32 *program, size_t program_len, size_t n_cols, size_t n_out, uint64_t *kernel_id) {
    TSTWO_REQUIRE_READY();
    if (!program || !kernel_id) return bad("null host argument");
    if (stream_is_capturing()) return bad("air columns compile: refused during graph capture (it loads a module, synchronously)");
    std::string src;
    if (const char *why = air_columns_codegen(program, program_len, n_cols, n_out, src)) return bad(std::string("air columns: ") + why);
    return compile_and_register(src, kAirKernelColumns, n_cols, n_out, kernel_id);
}

int tstwo_air_kernel_info(uint64_t kernel_id, u32 info[TSTWO_AIR_KERNEL_INFO_WORDS]) {
    TSTWO_REQUIRE_READY();
    if (!info) return bad("null host argument");
    const Kernel *k = find(kernel_id);
    if (!k) return bad("unknown air kernel");
    for (int w = 0; w < 2; w++) {
        int vgprs = 0, priv = 0;
        TSTWO_HIP(hipFuncGetAttribute(&vgprs, HIP_FUNC_ATTRIBUTE_NUM_REGS, k->fn[w]));
        TSTWO_HIP(hipFuncGetAttribute(&priv, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, k->fn[w]));
        info[3 * w] = (u32)vgprs;
        info[3 * w + 1] = k->sgprs[w];
        info[3 * w + 2] = (u32)priv;
    }
    info[6] = (u32)k->code_bytes;
    return TSTWO_OK;
}

int tstwo_air_program_destroy(uint64_t kernel_id) {
    TSTWO_REQUIRE_READY();
    Kernel *k = find(kernel_id);
    if (!k) return bad("unknown air kernel");
    if (stream_is_capturing()) return bad("air program destroy: refused during graph capture");
    TSTWO_HIP(hipStreamSynchronize(ctx().stream));         // a launch of it may still be running
    const hipModule_t module = k->module;
    g_kernels.erase(kernel_id);
    TSTWO_HIP(hipModuleUnload(module));
    return TSTWO_OK;
}

}  // extern "C"
