// Drives ORB_SLAM::KeyFrameDatabase (orb_slam_amd/cpp/KeyFrameDatabase.cc, over the stand-in KeyFrame.h / Frame.h of this
// directory) through a script of operations; tests/test_gpu_kfdb_dropin.py runs the same script through the Python restatement
// (tests/kfdb_ref.py) and compares the output line by line.
//
//   harness VOCABULARY.txt SCRIPT [serial|threads|churn]
//
// Script lines:
//   kf ID N w v ...      a KeyFrame with mnId = ID and a BowVector of N (word, value) pairs (values exact, %.17g)
//   cov ID M c1 .. cM    its covisible key frames, best first (GetConnectedKeyFrames is the same set)
//   set ID lq lw ls rq rw rs   the six database fields of key frame ID
//   add ID | erase ID | clear
//   loop ID MINSCORE     DetectLoopCandidates(kf ID, MINSCORE)            -> "R id id ..."
//   reloc ID N w v ...   DetectRelocalisationCandidates(Frame mnId = ID)  -> "R id id ..."
//   dump                 -> "D" and, per key frame in creation order, "id lq lw ls rq rw rs" (floats %.9g)
//   parallel / join      (churn) the lines in between run concurrently: add / erase on one writer thread, the searches
//                        alternately on two reader threads (their results are not printed)
// threads: the setup runs serially, then the loop searches run on three threads (search i on thread i % 3) and are printed
// as "Q i id id ..." in search order.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"

using namespace ORB_SLAM;

namespace {

std::map<unsigned long, std::unique_ptr<KeyFrame> > g_kfs;
std::vector<unsigned long> g_order;

void read_bow(std::istringstream& in, DBoW2::BowVector& v) {
    int n = 0;
    in >> n;
    v.clear();
    for (int i = 0; i < n; i++) {
        unsigned int w;
        std::string val;
        in >> w >> val;
        v[w] = strtod(val.c_str(), nullptr);
    }
}

std::string result(const std::vector<KeyFrame*>& r) {
    std::string s = "R";
    for (size_t i = 0; i < r.size(); i++) s += " " + std::to_string(r[i]->mnId);
    return s;
}

std::string dump() {
    std::string s = "D";
    char buf[256];
    for (size_t i = 0; i < g_order.size(); i++) {
        const KeyFrame* k = g_kfs[g_order[i]].get();
        snprintf(buf, sizeof buf, "\n%lu %lu %d %.9g %lu %d %.9g", k->mnId, k->mnLoopQuery, k->mnLoopWords, (double)k->mLoopScore,
                 k->mnRelocQuery, k->mnRelocWords, (double)k->mRelocScore);
        s += buf;
    }
    return s;
}

// one line; returns the text to print ("" for none)
std::string run(KeyFrameDatabase& db, const std::string& line) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    unsigned long id = 0;
    if (op == "kf") {
        in >> id;
        std::unique_ptr<KeyFrame>& k = g_kfs[id];
        if (!k) { k.reset(new KeyFrame); g_order.push_back(id); }
        k->mnId = id;
        read_bow(in, k->mBowVec);
    } else if (op == "cov") {
        int m = 0;
        in >> id >> m;
        KeyFrame* k = g_kfs[id].get();
        k->mvpOrderedConnectedKeyFrames.clear();
        for (int i = 0; i < m; i++) {
            unsigned long c;
            in >> c;
            k->mvpOrderedConnectedKeyFrames.push_back(g_kfs[c].get());
        }
    } else if (op == "set") {
        std::string ls, rs;
        in >> id;
        KeyFrame* k = g_kfs[id].get();
        in >> k->mnLoopQuery >> k->mnLoopWords >> ls >> k->mnRelocQuery >> k->mnRelocWords >> rs;
        k->mLoopScore = strtof(ls.c_str(), nullptr);
        k->mRelocScore = strtof(rs.c_str(), nullptr);
    } else if (op == "add") {
        in >> id;
        db.add(g_kfs.at(id).get());
    } else if (op == "erase") {
        in >> id;
        db.erase(g_kfs.at(id).get());
    } else if (op == "clear") {
        db.clear();
    } else if (op == "loop") {
        std::string ms;
        in >> id >> ms;
        return result(db.DetectLoopCandidates(g_kfs.at(id).get(), strtof(ms.c_str(), nullptr)));
    } else if (op == "reloc") {
        Frame f;
        in >> f.mnId;
        read_bow(in, f.mBowVec);
        return result(db.DetectRelocalisationCandidates(&f));
    } else if (op == "dump") {
        return dump();
    } else if (!op.empty()) {
        fprintf(stderr, "unknown line: %s\n", line.c_str());
        exit(2);
    }
    return "";
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s VOCABULARY.txt SCRIPT [serial|threads|churn]\n", argv[0]);
        return 2;
    }
    const std::string mode = argc > 3 ? argv[3] : "serial";
    ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    KeyFrameDatabase db(voc, 4096);
    std::ifstream f(argv[2]);
    std::vector<std::string> lines;
    for (std::string l; std::getline(f, l);) lines.push_back(l);

    if (mode == "threads") {
        std::vector<std::string> searches;
        for (size_t i = 0; i < lines.size(); i++) {
            if (lines[i].compare(0, 5, "loop ") == 0) searches.push_back(lines[i]);
            else run(db, lines[i]);
        }
        std::vector<std::string> out(searches.size());
        std::vector<std::thread> th;
        for (int t = 0; t < 3; t++)
            th.emplace_back([&, t]() { for (size_t i = t; i < searches.size(); i += 3) out[i] = run(db, searches[i]); });
        for (size_t t = 0; t < th.size(); t++) th[t].join();
        for (size_t i = 0; i < out.size(); i++) printf("Q %zu%s\n", i, out[i].c_str() + 1);
        return 0;
    }
    for (size_t i = 0; i < lines.size(); i++) {
        if (mode == "churn" && lines[i] == "parallel") {
            std::vector<std::string> writes, reads[2];
            size_t j = i + 1;
            for (int r = 0; j < lines.size() && lines[j] != "join"; j++) {
                if (lines[j].compare(0, 4, "add ") == 0 || lines[j].compare(0, 6, "erase ") == 0) writes.push_back(lines[j]);
                else reads[r++ & 1].push_back(lines[j]);
            }
            std::thread w([&]() { for (size_t k = 0; k < writes.size(); k++) run(db, writes[k]); });
            std::thread r0([&]() { for (size_t k = 0; k < reads[0].size(); k++) run(db, reads[0][k]); });
            std::thread r1([&]() { for (size_t k = 0; k < reads[1].size(); k++) run(db, reads[1][k]); });
            w.join();
            r0.join();
            r1.join();
            i = j;
            continue;
        }
        const std::string s = run(db, lines[i]);
        if (!s.empty()) printf("%s\n", s.c_str());
    }
    return 0;
}
