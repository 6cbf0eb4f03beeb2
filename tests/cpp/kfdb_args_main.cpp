// kfdb_args_main.cpp -- the host side of csrc/kfdb.hip on its own, for tests/test_kfdb.py: the argument
// checks (every one comes before the device is looked at), n == 0, and the carving of the opaque block
// from a null base, compiled for the host under the address and undefined-behaviour sanitizers.
// No HIP runtime is linked: the few names the host code refers to are defined here, and the device
// check answers that there is no device, so nothing is launched.
//   kfdb_args_main          runs the checks, prints "ok"
//   kfdb_args_main sizes    prints the size of every struct of orbgpu_kfdb.h and some offsets
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../orb-slam2-annotation_amd/csrc/kfdb.hip"

// ---- what liborbgpu.so and the HIP runtime would provide
namespace orbgpu {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int check_device() { return fail(ORBGPU_ERR_NO_DEVICE, "no device"); }
}  // namespace orbgpu

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int*) { return hipErrorNoDevice; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipErrorNoDevice; }
const char* hipGetErrorString(hipError_t) { return "no HIP runtime"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { return nullptr; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "kfdb_args_main: %s (line %d)\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static int sizes() {
    std::printf("orbgpu_kfdb %zu\n", sizeof(orbgpu_kfdb));
    std::printf("orbgpu_kfdb_query %zu\n", sizeof(orbgpu_kfdb_query));
    std::printf("orbgpu_kfdb_result %zu\n", sizeof(orbgpu_kfdb_result));
    std::printf("db.n_bow_total %zu\n", offsetof(orbgpu_kfdb, n_bow_total));
    std::printf("db.in_db %zu\n", offsetof(orbgpu_kfdb, in_db));
    std::printf("db.kf_bad %zu\n", offsetof(orbgpu_kfdb, kf_bad));
    std::printf("db.bow_values %zu\n", offsetof(orbgpu_kfdb, bow_values));
    std::printf("db.reloc_score %zu\n", offsetof(orbgpu_kfdb, reloc_score));
    std::printf("query.n_covisible %zu\n", offsetof(orbgpu_kfdb_query, n_covisible));
    std::printf("query.min_score %zu\n", offsetof(orbgpu_kfdb_query, min_score));
    std::printf("query.words %zu\n", offsetof(orbgpu_kfdb_query, words));
    std::printf("query.d_n_words %zu\n", offsetof(orbgpu_kfdb_query, d_n_words));
    std::printf("query.covisible %zu\n", offsetof(orbgpu_kfdb_query, covisible));
    std::printf("result.n_candidates %zu\n", offsetof(orbgpu_kfdb_result, n_candidates));
    std::printf("result.min_score %zu\n", offsetof(orbgpu_kfdb_result, min_score));
    std::printf("result.best_acc_score %zu\n", offsetof(orbgpu_kfdb_result, best_acc_score));
    std::printf("max_keyframes %d\n", ORBGPU_KFDB_MAX_KEYFRAMES);
    std::printf("max_words %d\n", ORBGPU_KFDB_MAX_WORDS);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sizes")) return sizes();
    char block[256];
    void* p = block;  // never dereferenced: every call below returns before the device is looked at, or finds none
    auto queries = static_cast<const orbgpu_kfdb_query*>(p);
    auto res = static_cast<orbgpu_kfdb_result*>(p);
    auto ip = static_cast<int*>(p);
    auto fp = static_cast<float*>(p);
    orbgpu_kfdb db;
    std::memset(&db, 0, sizeof(db));
    db.n_kf = 100;
    db.n_bow_total = 5000;
    auto call = [&](int n, const orbgpu_kfdb_query* q, const orbgpu_kfdb* d, int cs, void* ws, orbgpu_kfdb_result* r,
                    int* c) { return orbgpu_kfdb_detect_batch_device(n, q, d, cs, ws, r, c, ip, fp, nullptr); };
    EXPECT(call(1, queries, &db, 4, p, res, ip) == ORBGPU_ERR_NO_DEVICE);  // valid arguments reach the device check
    EXPECT(orbgpu_kfdb_detect_batch_device(1, queries, &db, 4, p, res, ip, nullptr, nullptr, nullptr) ==
           ORBGPU_ERR_NO_DEVICE);  // the rows are optional
    EXPECT(call(-1, queries, &db, 4, p, res, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, &db, 0, p, res, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, &db, -3, p, res, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, nullptr, 4, p, res, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, &db, 4, p, nullptr, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, &db, 4, p, res, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(call(1, nullptr, &db, 4, p, res, ip) == ORBGPU_ERR_ARG);
    EXPECT(call(1, queries, &db, 4, nullptr, res, ip) == ORBGPU_ERR_ARG);
    // n == 0 needs no device and no table, but what is given is still checked
    EXPECT(call(0, nullptr, nullptr, 4, nullptr, nullptr, nullptr) == ORBGPU_OK);
    EXPECT(call(0, nullptr, &db, 4, nullptr, res, ip) == ORBGPU_OK);
    EXPECT(call(0, nullptr, &db, 0, nullptr, res, ip) == ORBGPU_ERR_ARG);
    {
        orbgpu_kfdb d = db;
        d.n_kf = ORBGPU_KFDB_MAX_KEYFRAMES + 1;
        EXPECT(call(0, nullptr, &d, 4, nullptr, res, ip) == ORBGPU_ERR_ARG);
    }
    {
        orbgpu_kfdb d = db;
        d.n_kf = -1;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_ARG);
        d = db;
        d.n_bow_total = -1;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_ARG);
        d = db;
        d.n_kf = ORBGPU_KFDB_MAX_KEYFRAMES;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_NO_DEVICE);
        d.n_kf = ORBGPU_KFDB_MAX_KEYFRAMES + 1;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_ARG);
        d = db;
        d.scoring = 6;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_ARG);
        d.scoring = -1;
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_ARG);
        d = db;
        d.n_kf = 0;  // an empty database is valid
        EXPECT(call(1, queries, &d, 4, p, res, ip) == ORBGPU_ERR_NO_DEVICE);
    }
    static_assert(ORBGPU_KFDB_MAX_KEYFRAMES >= 8192, "the documented limit");
    // the glue
    auto cand = static_cast<orbgpu_reloc_candidate*>(p);
    auto rq = static_cast<orbgpu_reloc_query*>(p);
    auto bf = static_cast<orbgpu_bow_frame*>(p);
    auto u8 = static_cast<const uint8_t*>(p);
    auto emit = [&](int n, int cs, const int* f, const orbgpu_bow_frame* kb, orbgpu_bow_frame* a) {
        return orbgpu_kfdb_emit_reloc_batch_device(n, f, res, ip, cs, u8, kb, bf, cand, rq, a, bf, nullptr);
    };
    EXPECT(emit(2, 8, ip, bf, bf) == ORBGPU_ERR_NO_DEVICE);
    EXPECT(orbgpu_kfdb_emit_reloc_batch_device(2, ip, res, ip, 8, nullptr, bf, bf, cand, rq, bf, bf, nullptr) ==
           ORBGPU_ERR_NO_DEVICE);  // no keyframe is bad
    EXPECT(emit(-1, 8, ip, bf, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(2, 0, ip, bf, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(2, ORBGPU_LOOP_MAX_CANDIDATES, ip, bf, bf) == ORBGPU_ERR_NO_DEVICE);
    EXPECT(emit(2, ORBGPU_LOOP_MAX_CANDIDATES + 1, ip, bf, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(1 << 30, 8, ip, bf, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(2, 8, nullptr, bf, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(2, 8, ip, nullptr, bf) == ORBGPU_ERR_ARG);
    EXPECT(emit(2, 8, ip, bf, nullptr) == ORBGPU_ERR_ARG);
    EXPECT(emit(0, 8, nullptr, nullptr, nullptr) == ORBGPU_OK);
    // the carving: sizes from a null base grow with both dimensions and are 256-byte multiples
    size_t prev = 0;
    for (int n = 0; n <= 64; n += 8) {
        const size_t a = orbgpu_kfdb_detect_workspace_bytes(n, 100 * n);
        EXPECT(a > 0 && a % 256 == 0 && a >= prev);
        prev = a;
    }
    EXPECT(orbgpu_kfdb_detect_workspace_bytes(-5, -5) == orbgpu_kfdb_detect_workspace_bytes(1, 1));
    EXPECT(orbgpu_kfdb_detect_workspace_bytes(2, 0) == orbgpu_kfdb_detect_workspace_bytes(2, 1));
    EXPECT(orbgpu_kfdb_detect_workspace_bytes(64, ORBGPU_KFDB_MAX_KEYFRAMES) >= (size_t)64 * ORBGPU_KFDB_MAX_KEYFRAMES * 25);
    std::printf("ok\n");
    return 0;
}
