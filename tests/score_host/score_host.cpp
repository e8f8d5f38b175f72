// Caller of the C++ mirror's PoastaAligner::score_batch (include/poasta_amd.hpp), one-piece and two-piece: built by
// tests/test_score_only.py, which compares what it prints with align_batch of the same mirror.
//   score_host <msa.fa> <queries.fa>  ->  per query "score flags dense_score" under 4 / 6 / 2, then under 4 / 6,24 / 2,1
#include <cstdio>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/poasta_amd.hpp"

using namespace poasta;

static std::vector<std::pair<std::string, std::string>> read_fasta(const char* path) {
    std::vector<std::pair<std::string, std::string>> out;
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') out.push_back({line.substr(1), std::string()});
        else if (!out.empty()) out.back().second += line;
    }
    return out;
}

template <typename Config>
static int run(const graphs::POAGraph& g, const std::vector<std::string>& seqs, Config cfg) {
    aligner::PoastaAligner<Config> al(cfg, aligner::AlignmentType::Global);
    const auto sc = al.score_batch(g, seqs);
    const auto full = al.align_batch(g, seqs);
    for (size_t i = 0; i < seqs.size(); ++i) {
        if (!sc[i].alignment.empty()) return 2;
        std::printf("%u %u %u\n", sc[i].score, sc[i].flags, full[i].score);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    try {
        graphs::POAGraph g = io::load_graph_from_fasta_msa(read_fasta(argv[1]));
        std::vector<std::string> seqs;
        for (auto& r : read_fasta(argv[2])) seqs.push_back(r.second);
        int rc = run(g, seqs, aligner::AffineMinGapCost(aligner::GapAffine(4, 2, 6)));
        if (rc) return rc;
        return run(g, seqs, aligner::Affine2PieceDijkstra(aligner::GapAffine2Piece(4, 2, 6, 1, 24)));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "score_host: %s\n", e.what());
        return 1;
    }
}
