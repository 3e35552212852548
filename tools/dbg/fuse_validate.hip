// fuse_validate.hip — host-side sanitizer check of the argument validation of orbfe_fuse_search and
// orbfe_scw_search.
//
// A program of its own: it links orbfe_fuse.hip alone and calls the entries only with arguments that the validation
// refuses (or with nothing to do), all of which return before any device call, so it runs on a machine without a
// GPU.  What orbfe_scw_search accepts where orbfe_fuse_search refuses (a null blocked, anything in slot 4 of the
// keyframe scalars) would reach the device on its own, so each is paired with one later refusal and the message must
// be that later one's.  Build and run with tools/dbg/fuse_validate_asan.sh (host code under
// -fsanitize=address,undefined).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../../include/orbfe.h"

namespace orbfe {
thread_local std::string g_err;
}

namespace {

struct Input {
    // one keyframe with a 2 x 2 grid and two features, two levels, two points
    std::vector<double> kf = std::vector<double>(ORBFE_FUSE_KF_F64, 1.0);
    std::vector<int32_t> ki = {2, 2, 2};
    std::vector<int64_t> off = {0, 2}, cell_at = {0, 5}, idx_at = {0, 2}, lvl_off = {0, 2};
    std::vector<double> xy = {1.0, 1.0, 2.0, 2.0}, ur = {-1.0, 0.5}, scale = {1.0, 1.2}, is2 = {1.0, 0.7};
    std::vector<int32_t> octave = {0, 1}, cell_off = {0, 1, 1, 2, 2}, cell_idx = {0, 1};
    std::vector<uint8_t> desc = std::vector<uint8_t>(64, 7), pdesc = std::vector<uint8_t>(64, 9), blocked = {0, 1};
    std::vector<double> pt = std::vector<double>(2 * ORBFE_FUSE_PT_F64, 1.0);
    std::vector<int32_t> bi = {-7, -7}, bd = {-7, -7};
    std::vector<uint8_t> st = {7, 7};
    int32_t n_kf = 1;
    int64_t n_pts = 2, stride = 2;
    double th = 3.0, eps = 0x1p-48;
    bool null_out = false;
    const void* skip = nullptr;  // the array passed as a null pointer

    template <class T>
    const T* p(const std::vector<T>& v) const {
        return v.data() == skip ? nullptr : v.data();
    }
    template <class T>
    T* p(std::vector<T>& v) {
        return v.data() == skip ? nullptr : v.data();
    }
    int run(bool scw) {
        if (scw) {  // no ur, no is2
            orbfe_scw_out o{p(bi), p(bd), p(st)};
            return orbfe_scw_search(p(kf), p(ki), p(off), p(xy), p(octave), p(desc), p(blocked), p(cell_at),
                                    p(cell_off), p(idx_at), p(cell_idx), p(lvl_off), p(scale), n_kf, p(pt), p(pdesc),
                                    n_pts, th, eps, null_out ? nullptr : &o, stride);
        }
        orbfe_fuse_out o{p(bi), p(bd), p(st)};
        return orbfe_fuse_search(p(kf), p(ki), p(off), p(xy), p(octave), p(ur), p(desc), p(cell_at), p(cell_off),
                                 p(idx_at), p(cell_idx), p(lvl_off), p(scale), p(is2), n_kf, p(pt), p(pdesc), n_pts, th,
                                 eps, null_out ? nullptr : &o, stride);
    }
    bool untouched() const { return bi[0] == -7 && bi[1] == -7 && bd[0] == -7 && bd[1] == -7 && st[0] == 7 && st[1] == 7; }
};

int failures = 0, checks = 0;
bool scw = false;  // the entry under test

// message: words the refusal's message must hold ("" for any)
void expect(const char* what, int want, const std::function<void(Input&)>& breakit, const char* message = "") {
    Input in;
    breakit(in);
    orbfe::g_err.clear();
    const int rc = in.run(scw);
    ++checks;
    if (rc != want || !in.untouched() || orbfe::g_err.find(message) == std::string::npos) {
        std::printf("FAIL %s %s: rc %d (want %d), outputs %s, message: %s (want: %s)\n", scw ? "scw" : "fuse", what, rc,
                    want, in.untouched() ? "untouched" : "WRITTEN", orbfe::g_err.c_str(), message);
        ++failures;
    }
}

void refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int E = ORBFE_EINVAL;
    expect("negative keyframe count", E, [](Input& i) { i.n_kf = -1; });
    expect("negative point count", E, [](Input& i) { i.n_pts = -1; });
    expect("negative stride", E, [](Input& i) { i.stride = -1; });
    expect("too many keyframes", E, [](Input& i) { i.n_kf = 65536; });
    expect("th nan", E, [&](Input& i) { i.th = nan; });
    expect("eps inf", E, [&](Input& i) { i.eps = inf; });
    expect("eps negative", E, [](Input& i) { i.eps = -1.0; });
    expect("no keyframes", ORBFE_OK, [](Input& i) { i.n_kf = 0; });
    expect("no points", ORBFE_OK, [](Input& i) { i.n_pts = 0; });
    expect("null out", E, [](Input& i) { i.null_out = true; });
#define NULLARG(field) expect("null " #field, E, [](Input& i) { i.skip = i.field.data(); }, "null argument")
    NULLARG(kf);
    NULLARG(ki);
    NULLARG(off);
    NULLARG(xy);
    NULLARG(octave);
    NULLARG(desc);
    NULLARG(cell_at);
    NULLARG(cell_off);
    NULLARG(idx_at);
    NULLARG(cell_idx);
    NULLARG(lvl_off);
    NULLARG(scale);
    NULLARG(pt);
    NULLARG(pdesc);
    NULLARG(bi);
    NULLARG(bd);
    NULLARG(st);
    expect("stride below the point count", E, [](Input& i) { i.stride = 1; });
    expect("off[0] not 0", E, [](Input& i) { i.off[0] = 1; });
    expect("offsets decrease", E, [](Input& i) { i.off[1] = -1; });
    expect("cell offsets decrease", E, [](Input& i) { i.cell_at[1] = -2; });
    expect("frame above the cap", E, [](Input& i) { i.off[1] = ORBFE_BOW_MAX_FRAME + 1; });
    expect("grid entries above the cap", E, [](Input& i) { i.idx_at[1] = ORBFE_BOW_MAX_FRAME + 1; });
    expect("level count 0", E, [](Input& i) { i.ki[2] = 0; });
    expect("level count negative", E, [](Input& i) { i.ki[2] = -5; });
    expect("level table of another length", E, [](Input& i) { i.ki[2] = 1; }, "one entry per level");
    expect("no grid columns", E, [](Input& i) { i.ki[0] = 0; });
    expect("huge grid", E, [](Input& i) { i.ki[1] = 1 << 30; });
    expect("grid offsets not columns * rows + 1", E, [](Input& i) { i.ki[0] = 3; });
    expect("first cell offset", E, [](Input& i) { i.cell_off[0] = 1; });
    expect("cell offsets not monotone", E, [](Input& i) { i.cell_off[2] = 0; });
    expect("last cell offset", E, [](Input& i) { i.cell_off[4] = 3; });
    expect("grid entry past the features", E, [](Input& i) { i.cell_idx[1] = 2; });
    expect("grid entry negative", E, [](Input& i) { i.cell_idx[0] = -1; });
    expect("octave past the levels", E, [](Input& i) { i.octave[1] = 2; });
    expect("octave negative", E, [](Input& i) { i.octave[0] = -1; });
    for (int c = 0; c < ORBFE_FUSE_KF_F64; ++c) {
        if (scw && c == 4) continue;  // bf: not read, see below
        expect("keyframe scalar nan", E, [&](Input& i) { i.kf[c] = nan; }, "a scalar is not finite");
        expect("keyframe scalar inf", E, [&](Input& i) { i.kf[c] = -inf; }, "a scalar is not finite");
    }
    for (int c = 0; c < 2 * ORBFE_FUSE_PT_F64; ++c) expect("point scalar nan", E, [&](Input& i) { i.pt[c] = nan; });
    expect("coordinate inf", E, [&](Input& i) { i.xy[3] = inf; });
    expect("scale nan", E, [&](Input& i) { i.scale[1] = nan; });
    if (scw) {
        // accepted by the validation: the refusal is the later one, of the point scalar
        const char* later = "a point scalar is not finite";
        expect("null blocked goes on", E, [&](Input& i) { i.skip = i.blocked.data(), i.pt[0] = nan; }, later);
        expect("bf nan goes on", E, [&](Input& i) { i.kf[4] = nan, i.pt[0] = nan; }, later);
        expect("bf inf goes on", E, [&](Input& i) { i.kf[4] = -inf, i.pt[0] = nan; }, later);
    } else {
        NULLARG(ur);
        NULLARG(is2);
        expect("right coordinate nan", E, [&](Input& i) { i.ur[0] = nan; });
        expect("inverse sigma inf", E, [&](Input& i) { i.is2[0] = inf; });
    }
    float ms = -1.f;
    const auto last_ms = scw ? orbfe_scw_search_last_ms : orbfe_fuse_search_last_ms;
    if (last_ms(nullptr) != E || last_ms(&ms) != ORBFE_OK || ms != 0.f) {
        std::printf("FAIL %s last_ms\n", scw ? "scw" : "fuse");
        ++failures;
    }
}

}  // namespace

int main() {
    for (bool s : {false, true}) {
        scw = s;
        refusals();
    }
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
