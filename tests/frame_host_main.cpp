// Driver of tests/test_frame_host.py for eqf_vio_amd/csrc/eqf_frame.hpp (host only: built with g++ and the sanitizers, no GPU, no HIP).
// Cases arrive on stdin as whitespace-separated tokens, results leave on stdout as lines of integers; the expected values are computed in
// Python, never by this header.  A scene is `B cap` and per filter `active nIds id.. nMeas measId..`.  The three `history` routes replay
// frames the way eqf_capi.hip drives the header: the chords a kernel would have written are made from the frame's list of outlier ids.
// `layout B cap` prints frame::ImageLayout: bearingStride bearingDoubles offKeep offPerm offCounts editInts offEdit doubles.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "eqf_frame.hpp"

using namespace eqf::frame;

namespace {

std::string token() {
    std::string s;
    if (!(std::cin >> s)) std::exit(3);
    return s;
}
int readInt() { return std::atoi(token().c_str()); }
double readDouble() { return std::strtod(token().c_str(), nullptr); }  // (accepts "nan")
std::vector<int> readList() {
    std::vector<int> v(readInt());
    for (int& x : v) x = readInt();
    return v;
}
void put(const std::vector<int>& v) {
    for (int x : v) std::printf("%d ", x);
    std::printf("\n");
}
void put(const Lists& l) {
    for (auto& v : l) put(v);
}
void putMarks(const Marks& mk) {  // the marked indices
    for (auto& v : mk) {
        for (size_t k = 0; k < v.size(); ++k)
            if (v[k]) std::printf("%d ", int(k));
        std::printf("\n");
    }
}

struct Scene {
    int B = 0, cap = 0;
    Lists ids, meas;
    std::vector<char> active;
    std::vector<const int*> mptr;
    std::vector<int> nb;
    void readMeas(int b) {
        active[b] = char(readInt());
        meas[b] = readList();
    }
    void point() {
        mptr.resize(B);
        nb.resize(B);
        for (int b = 0; b < B; ++b) mptr[b] = meas[b].data(), nb[b] = int(meas[b].size());
    }
    void read() {
        B = readInt(), cap = readInt();
        ids.resize(B), meas.resize(B), active.resize(B);
        for (int b = 0; b < B; ++b) {
            active[b] = char(readInt());
            ids[b] = readList();
            meas[b] = readList();
        }
        point();
    }
    Meas m() const { return Meas{mptr, nb, active}; }
};

std::vector<double> readChords(const Scene& s) {  // per filter as many as it has landmarks, at [b * cap + i]
    std::vector<double> c((size_t)s.B * s.cap, 0.0);
    for (int b = 0; b < s.B; ++b)
        for (size_t i = 0; i < s.ids[b].size(); ++i) c[(size_t)b * s.cap + i] = readDouble();
    return c;
}

// addNewLandmarks as eqf_capi.hip's addNewAndUpdate does it
void appendFresh(Scene& s, const std::vector<char>& active, const Lists& perm, const Marks* dropped) {
    for (int b = 0; b < s.B; ++b)
        if (active[b])
            forUnmatched(perm[b].data(), int(perm[b].size()), s.nb[b], dropped ? (*dropped)[b].data() : nullptr,
                [&](int k) { s.ids[b].push_back(s.meas[b][k]); });
}

bool isOut(const std::vector<int>& out, int id) { return std::find(out.begin(), out.end(), id) != out.end(); }

// one frame of a history; route 0 synchronous gate, 1 speculative probe + host redo, 2 k_edit with the gate on the device (a frame that is
// not eligible takes route 1, as in visionCore).  Returns the route taken.
int historyFrame(Scene& s, int route, double thr, int editMax, int editSafeN, const Lists& out) {
    const Meas m = s.m();
    Lists keep, perm;
    const bool anyLost = keepPresent(s.ids, m, keep);
    size_t maxN = 0;
    for (auto& v : s.ids) maxN = std::max(maxN, v.size());
    const bool gateArmed = thr < 2.0 && maxN > 0;
    std::vector<double> chord((size_t)s.B * s.cap, 0.0);
    std::vector<int> flag(s.B, 0);
    if (route == 2) {
        const EditChoice e = editEligible(s.ids, keep, m, true, gateArmed, editMax, editSafeN);
        if (e.ok && (anyLost || e.anyFresh || gateArmed)) {
            std::vector<int> image(ImageLayout{size_t(s.B), size_t(s.cap)}.editInts());
            EditPlan plan;
            if (!editImage(s.ids, keep, m, gateArmed, s.cap, image.data(), plan)) std::exit(4);
            s.ids = plan.newIds;
            if (!gateArmed) return 2;
            for (int b = 0; b < s.B; ++b) {  // what k_edit leaves: chords of the kept landmarks, flag 1 (2: the filter became too small)
                int nOut = 0;
                for (int j = 0; j < plan.nKept[b]; ++j)
                    if (s.active[b] && isOut(out[b], s.ids[b][j])) chord[(size_t)b * s.cap + j] = 1.0, ++nOut;
                if (nOut) flag[b] = int(s.ids[b].size()) - nOut < editSafeN ? 2 : 1;
            }
            gateOnDevice(s.ids, flag.data(), s.active, plan.nKept, chord.data(), s.cap, thr);
            return 2;
        }
        route = 1;
    }
    if (anyLost) applyKeep(s.ids, keep);
    matchPerm(s.ids, m, perm);
    Marks dropped(s.B);
    for (int b = 0; b < s.B; ++b) dropped[b].assign(s.nb[b], 0);
    maxN = 0;
    for (auto& v : s.ids) maxN = std::max(maxN, v.size());
    if (thr < 2.0 && maxN > 0) {
        for (int b = 0; b < s.B; ++b)  // what k_probe leaves
            for (size_t i = 0; i < s.ids[b].size(); ++i)
                if (s.active[b] && isOut(out[b], s.ids[b][i])) chord[(size_t)b * s.cap + i] = 1.0, flag[b] = 1;
        if (route == 0) {
            if (gateSync(s.ids, perm, s.active, chord.data(), s.cap, thr, keep, dropped)) {
                applyKeep(s.ids, keep);
                matchPerm(s.ids, m, perm);
            }
        } else {
            std::vector<int> nOld(s.B);
            for (int b = 0; b < s.B; ++b) nOld[b] = int(s.ids[b].size());
            appendFresh(s, s.active, perm, nullptr);  // (the frame goes on without the answer ...)
            std::vector<char> act;
            Marks gated;
            if (!gateRedo(s.ids, flag.data(), s.active, s.meas, s.nb, nOld, chord.data(), s.cap, thr, act, keep, gated)) return 1;
            applyKeep(s.ids, keep);  // (... and is redone for the flagged filters: resolveGate, then visionCore with `gated`)
            const Meas redo{s.mptr, s.nb, act};
            if (keepPresent(s.ids, redo, keep)) std::exit(5);
            matchPerm(s.ids, redo, perm);
            appendFresh(s, act, perm, &gated);
            return 1;
        }
    }
    appendFresh(s, s.active, perm, &dropped);
    return route;
}

}  // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "history") {
            Scene s;
            const int route = readInt();
            s.B = readInt(), s.cap = readInt();
            const double thr = readDouble();
            const int editMax = readInt(), editSafeN = readInt(), F = readInt();
            s.ids.resize(s.B), s.meas.resize(s.B), s.active.resize(s.B);
            for (int fr = 0; fr < F; ++fr) {
                Lists out(s.B);
                for (int b = 0; b < s.B; ++b) {
                    s.readMeas(b);
                    out[b] = readList();
                }
                s.point();
                std::printf("%d\n", historyFrame(s, route, thr, editMax, editSafeN, out));
                put(s.ids);
            }
            continue;
        }
        if (cmd == "layout") {
            const size_t B = size_t(readInt()), cap = size_t(readInt());
            const ImageLayout l{B, cap};
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", l.bearingStride(), l.bearingDoubles(), l.offKeep(), l.offPerm(), l.offCounts(),
                l.editInts(), l.offEdit(), l.doubles());
            continue;
        }
        Scene s;
        s.read();
        const Meas m = s.m();
        Lists keep, perm;
        if (cmd == "keep") {
            std::printf("%d\n", int(keepPresent(s.ids, m, keep)));
            put(keep);
            applyKeep(s.ids, keep);
            put(s.ids);
        } else if (cmd == "perm") {
            Marks dropped(s.B);
            for (int b = 0; b < s.B; ++b) {
                dropped[b].assign(s.nb[b], 0);
                for (int k : readList()) dropped[b][k] = 1;
            }
            matchPerm(s.ids, m, perm);
            put(perm);
            std::printf("%d %d\n", int(isIdentity(perm)), int(isIdentity(perm, &s.active)));
            for (const Marks* d : {(const Marks*)nullptr, (const Marks*)&dropped})
                for (int b = 0; b < s.B; ++b) {
                    std::vector<int> un;
                    forUnmatched(perm[b].data(), int(perm[b].size()), s.nb[b], d ? (*d)[b].data() : nullptr, [&](int k) { un.push_back(k); });
                    put(un);
                }
        } else if (cmd == "edit") {
            const bool handleOk = readInt(), gateArmed = readInt();
            const int editMax = readInt(), editSafeN = readInt();
            const bool anyLost = keepPresent(s.ids, m, keep);
            const EditChoice e = editEligible(s.ids, keep, m, handleOk, gateArmed, editMax, editSafeN);
            // (exactly editInts() ints are the image: every one of them is written, and the canary behind them is not)
            const size_t nInts = ImageLayout{size_t(s.B), size_t(s.cap)}.editInts(), nCanary = 4;
            std::vector<int> image(nInts + nCanary, 12345);
            EditPlan plan;
            const bool ok = editImage(s.ids, keep, m, gateArmed, s.cap, image.data(), plan);
            for (size_t k = nInts; k < image.size(); ++k)
                if (image[k] != 12345) std::exit(6);
            image.resize(nInts);
            std::printf("%d %d %d %d\n", int(e.ok), int(e.anyFresh), int(anyLost), int(ok));
            if (!ok) continue;
            std::printf("%d %d\n", int(plan.anyWork), plan.Nmax);
            put(image);
            put(plan.newIds);
            put(plan.nKept);
            put(plan.skipped);
        } else if (cmd == "gatesync") {
            const double thr = readDouble();
            const std::vector<double> chord = readChords(s);
            matchPerm(s.ids, m, perm);
            keep.resize(s.B);
            Marks dropped(s.B);
            for (int b = 0; b < s.B; ++b) dropped[b].assign(s.nb[b], 0);
            std::printf("%d\n", int(gateSync(s.ids, perm, s.active, chord.data(), s.cap, thr, keep, dropped)));
            put(keep);
            putMarks(dropped);
        } else if (cmd == "gateredo" || cmd == "gatedev") {
            const double thr = readDouble();
            std::vector<int> flag(s.B), count(s.B);  // count: nOld (redo) / nKept (device)
            for (int b = 0; b < s.B; ++b) flag[b] = readInt(), count[b] = readInt();
            const std::vector<double> chord = readChords(s);
            if (cmd == "gatedev") {
                const DeviceGate d = gateOnDevice(s.ids, flag.data(), s.active, count, chord.data(), s.cap, thr);
                put(s.ids);
                put(flag);
                std::printf("%d %d\n", int(d.deferred), d.Nmax);
                continue;
            }
            std::vector<char> act;
            Marks gated;
            const bool any = gateRedo(s.ids, flag.data(), s.active, s.meas, s.nb, count, chord.data(), s.cap, thr, act, keep, gated);
            std::printf("%d\n", int(any));
            put(flag);
            put(std::vector<int>(act.begin(), act.end()));
            if (!any) continue;
            put(keep);
            putMarks(gated);
        } else {
            return 2;
        }
    }
    return 0;
}
