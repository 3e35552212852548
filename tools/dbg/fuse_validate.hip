// fuse_validate.hip — host-side sanitizer check of the argument validation of orbfe_fuse_search,
// orbfe_scw_search, orbfe_sim3_search and orbfe_fkf_search.
//
// A program of its own: it links orbfe_fuse.hip alone and calls the entries only with arguments that the validation
// refuses (or with nothing to do), all of which return before any device call, so it runs on a machine without a
// GPU.  What orbfe_scw_search accepts where orbfe_fuse_search refuses (a null blocked, anything in slot 4 of the
// keyframe scalars) would reach the device on its own, so each is paired with one later refusal and the message must
// be that later one's; likewise for what orbfe_sim3_search accepts (anything in slots 0-19 of a keyframe's scalars
// and in the normal of a point) and orbfe_fkf_search (a null blocked, slot 4, the normal).  Build and run with tools/dbg/fuse_validate_asan.sh (host code under
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

// orbfe_sim3_search: Input's keyframe and points, three searches (two items, none, one item)
struct Sim3Input : Input {
    std::vector<double> sf = std::vector<double>(3 * ORBFE_SIM3_F64, 0.5);
    std::vector<int32_t> skf = {0, 0, 0}, item = {1, 0, 1};
    std::vector<int64_t> soff = {0, 2, 2, 3};
    std::vector<int32_t> bi3 = {-7, -7, -7}, bd3 = {-7, -7, -7};
    std::vector<uint8_t> st3 = {7, 7, 7};
    int32_t n_srch = 3;

    int run3() {
        orbfe_sim3_out o{p(bi3), p(bd3), p(st3)};
        return orbfe_sim3_search(p(kf), p(ki), p(off), p(xy), p(octave), p(desc), p(cell_at), p(cell_off), p(idx_at),
                                 p(cell_idx), p(lvl_off), p(scale), n_kf, p(pt), p(pdesc), n_pts, p(sf), p(skf),
                                 p(soff), n_srch, p(item), th, eps, null_out ? nullptr : &o);
    }
    bool untouched3() const {
        for (int i = 0; i < 3; ++i)
            if (bi3[i] != -7 || bd3[i] != -7 || st3[i] != 7) return false;
        return true;
    }
};

void expect3(const char* what, int want, const std::function<void(Sim3Input&)>& breakit, const char* message = "") {
    Sim3Input in;
    breakit(in);
    orbfe::g_err.clear();
    const int rc = in.run3();
    ++checks;
    if (rc != want || !in.untouched3() || orbfe::g_err.find(message) == std::string::npos) {
        std::printf("FAIL sim3 %s: rc %d (want %d), outputs %s, message: %s (want: %s)\n", what, rc, want,
                    in.untouched3() ? "untouched" : "WRITTEN", orbfe::g_err.c_str(), message);
        ++failures;
    }
}

void sim3_refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int E = ORBFE_EINVAL;
    expect3("negative keyframe count", E, [](Sim3Input& i) { i.n_kf = -1; });
    expect3("negative point count", E, [](Sim3Input& i) { i.n_pts = -1; });
    expect3("negative search count", E, [](Sim3Input& i) { i.n_srch = -1; });
    expect3("too many keyframes", E, [](Sim3Input& i) { i.n_kf = 65536; });
    expect3("th nan", E, [&](Sim3Input& i) { i.th = nan; });
    expect3("eps negative", E, [](Sim3Input& i) { i.eps = -1.0; });
    expect3("no searches", ORBFE_OK, [](Sim3Input& i) { i.n_srch = 0; });
    expect3("no items", ORBFE_OK, [](Sim3Input& i) { i.soff = {0, 0, 0, 0}; });
    expect3("null out", E, [](Sim3Input& i) { i.null_out = true; });
#define NULL3(field) expect3("null " #field, E, [](Sim3Input& i) { i.skip = i.field.data(); }, "null argument")
    NULL3(kf);
    NULL3(ki);
    NULL3(off);
    NULL3(xy);
    NULL3(octave);
    NULL3(desc);
    NULL3(cell_at);
    NULL3(cell_off);
    NULL3(idx_at);
    NULL3(cell_idx);
    NULL3(lvl_off);
    NULL3(scale);
    NULL3(pt);
    NULL3(pdesc);
    NULL3(sf);
    NULL3(skf);
    NULL3(soff);
    NULL3(item);
    NULL3(bi3);
    NULL3(bd3);
    NULL3(st3);
    expect3("srch_off[0] not 0", E, [](Sim3Input& i) { i.soff[0] = 1; }, "srch_off[0]");
    expect3("srch_off decreases", E, [](Sim3Input& i) { i.soff[2] = 1; }, "search 1");
    expect3("target past the keyframes", E, [](Sim3Input& i) { i.skf[2] = 1; }, "search 2");
    expect3("target negative", E, [](Sim3Input& i) { i.skf[0] = -1; }, "search 0");
    expect3("item past the points", E, [](Sim3Input& i) { i.item[2] = 2; }, "outside the point table");
    expect3("item negative", E, [](Sim3Input& i) { i.item[0] = -1; }, "outside the point table");
    for (int c = 0; c < 3 * ORBFE_SIM3_F64; ++c)
        expect3("search scalar nan", E, [&](Sim3Input& i) { i.sf[c] = c % 2 ? nan : -inf; }, "a scalar is not finite");
    expect3("off[0] not 0", E, [](Sim3Input& i) { i.off[0] = 1; });
    expect3("level count 0", E, [](Sim3Input& i) { i.ki[2] = 0; });
    expect3("grid entry past the features", E, [](Sim3Input& i) { i.cell_idx[1] = 2; });
    expect3("octave negative", E, [](Sim3Input& i) { i.octave[0] = -1; });
    expect3("coordinate inf", E, [&](Sim3Input& i) { i.xy[3] = inf; });
    expect3("scale nan", E, [&](Sim3Input& i) { i.scale[1] = nan; });
    for (int c = 20; c < ORBFE_FUSE_KF_F64; ++c)
        expect3("keyframe scalar nan", E, [&](Sim3Input& i) { i.kf[c] = nan; }, "a scalar is not finite");
    const char* later = "a point scalar is not finite";
    for (int c = 0; c < 2 * ORBFE_FUSE_PT_F64; ++c) {
        if (c % ORBFE_FUSE_PT_F64 >= 3 && c % ORBFE_FUSE_PT_F64 < 6) continue;  // the normal: not read, see below
        expect3("point scalar nan", E, [&](Sim3Input& i) { i.pt[c] = nan; }, later);
    }
    // accepted by the validation: the refusal is the later one, of the point scalar
    for (int c = 0; c < 20; ++c)
        expect3("unread keyframe slot goes on", E, [&](Sim3Input& i) { i.kf[c] = nan, i.pt[8] = inf; }, later);
    for (int c = 3; c < 6; ++c)
        expect3("normal goes on", E, [&](Sim3Input& i) { i.pt[c] = -inf, i.pt[ORBFE_FUSE_PT_F64] = nan; }, later);
    float ms = -1.f;
    if (orbfe_sim3_search_last_ms(nullptr) != E || orbfe_sim3_search_last_ms(&ms) != ORBFE_OK || ms != 0.f) {
        std::printf("FAIL sim3 last_ms\n");
        ++failures;
    }
}

// orbfe_fkf_search: Sim3Input without the search scalars, with blocked
struct FkfInput : Sim3Input {
    int runf() {
        orbfe_fkf_out o{p(bi3), p(bd3), p(st3)};
        return orbfe_fkf_search(p(kf), p(ki), p(off), p(xy), p(octave), p(desc), p(blocked), p(cell_at), p(cell_off),
                                p(idx_at), p(cell_idx), p(lvl_off), p(scale), n_kf, p(pt), p(pdesc), n_pts, p(skf),
                                p(soff), n_srch, p(item), th, eps, null_out ? nullptr : &o);
    }
};

void expectf(const char* what, int want, const std::function<void(FkfInput&)>& breakit, const char* message = "") {
    FkfInput in;
    breakit(in);
    orbfe::g_err.clear();
    const int rc = in.runf();
    ++checks;
    if (rc != want || !in.untouched3() || orbfe::g_err.find(message) == std::string::npos) {
        std::printf("FAIL fkf %s: rc %d (want %d), outputs %s, message: %s (want: %s)\n", what, rc, want,
                    in.untouched3() ? "untouched" : "WRITTEN", orbfe::g_err.c_str(), message);
        ++failures;
    }
}

void fkf_refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int E = ORBFE_EINVAL;
    expectf("negative keyframe count", E, [](FkfInput& i) { i.n_kf = -1; });
    expectf("negative point count", E, [](FkfInput& i) { i.n_pts = -1; });
    expectf("negative search count", E, [](FkfInput& i) { i.n_srch = -1; });
    expectf("too many keyframes", E, [](FkfInput& i) { i.n_kf = 65536; });
    expectf("th nan", E, [&](FkfInput& i) { i.th = nan; });
    expectf("eps negative", E, [](FkfInput& i) { i.eps = -1.0; });
    expectf("no searches", ORBFE_OK, [](FkfInput& i) { i.n_srch = 0; });
    expectf("no items", ORBFE_OK, [](FkfInput& i) { i.soff = {0, 0, 0, 0}; });
    expectf("null out", E, [](FkfInput& i) { i.null_out = true; });
#define NULLF(field) expectf("null " #field, E, [](FkfInput& i) { i.skip = i.field.data(); }, "null argument")
    NULLF(kf);
    NULLF(ki);
    NULLF(off);
    NULLF(xy);
    NULLF(octave);
    NULLF(desc);
    NULLF(cell_at);
    NULLF(cell_off);
    NULLF(idx_at);
    NULLF(cell_idx);
    NULLF(lvl_off);
    NULLF(scale);
    NULLF(pt);
    NULLF(pdesc);
    NULLF(skf);
    NULLF(soff);
    NULLF(item);
    NULLF(bi3);
    NULLF(bd3);
    NULLF(st3);
    expectf("srch_off[0] not 0", E, [](FkfInput& i) { i.soff[0] = 1; }, "srch_off[0]");
    expectf("srch_off decreases", E, [](FkfInput& i) { i.soff[2] = 1; }, "search 1");
    expectf("target past the keyframes", E, [](FkfInput& i) { i.skf[2] = 1; }, "search 2");
    expectf("target negative", E, [](FkfInput& i) { i.skf[0] = -1; }, "search 0");
    expectf("item past the points", E, [](FkfInput& i) { i.item[2] = 2; }, "outside the point table");
    expectf("item negative", E, [](FkfInput& i) { i.item[0] = -1; }, "outside the point table");
    expectf("off[0] not 0", E, [](FkfInput& i) { i.off[0] = 1; });
    expectf("frame above the cap", E, [](FkfInput& i) { i.off[1] = ORBFE_BOW_MAX_FRAME + 1; });
    expectf("level count 0", E, [](FkfInput& i) { i.ki[2] = 0; });
    expectf("grid entry past the features", E, [](FkfInput& i) { i.cell_idx[1] = 2; });
    expectf("octave negative", E, [](FkfInput& i) { i.octave[0] = -1; });
    expectf("coordinate inf", E, [&](FkfInput& i) { i.xy[3] = inf; });
    expectf("scale nan", E, [&](FkfInput& i) { i.scale[1] = nan; });
    for (int c = 0; c < ORBFE_FUSE_KF_F64; ++c) {
        if (c == 4) continue;  // bf: not read, see below
        expectf("frame scalar nan", E, [&](FkfInput& i) { i.kf[c] = c % 2 ? nan : -inf; }, "a scalar is not finite");
    }
    const char* later = "a point scalar is not finite";
    for (int c = 0; c < 2 * ORBFE_FUSE_PT_F64; ++c) {
        if (c % ORBFE_FUSE_PT_F64 >= 3 && c % ORBFE_FUSE_PT_F64 < 6) continue;  // the normal: not read, see below
        expectf("point scalar nan", E, [&](FkfInput& i) { i.pt[c] = nan; }, later);
    }
    // accepted by the validation: the refusal is the later one, of the point scalar
    expectf("null blocked goes on", E, [&](FkfInput& i) { i.skip = i.blocked.data(), i.pt[0] = nan; }, later);
    expectf("bf nan goes on", E, [&](FkfInput& i) { i.kf[4] = nan, i.pt[0] = nan; }, later);
    for (int c = 3; c < 6; ++c)
        expectf("normal goes on", E, [&](FkfInput& i) { i.pt[c] = -inf, i.pt[ORBFE_FUSE_PT_F64] = nan; }, later);
    float ms = -1.f;
    if (orbfe_fkf_search_last_ms(nullptr) != E || orbfe_fkf_search_last_ms(&ms) != ORBFE_OK || ms != 0.f) {
        std::printf("FAIL fkf last_ms\n");
        ++failures;
    }
}

}  // namespace

int main() {
    for (bool s : {false, true}) {
        scw = s;
        refusals();
    }
    sim3_refusals();
    fkf_refusals();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
