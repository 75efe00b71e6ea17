// Stand-alone driver of csrc/host_exchange.h (tests/test_host_exchange.py compiles it with the address and undefined-
// behaviour sanitizers and runs it as an ordinary program; no GPU, no Python).
//
//   host_exchange_driver PREFIX ID WORLD sleep|spin CAP TIMEOUT_S MISSING N_0 N_1 ...
//
// forks WORLD processes (rank MISSING, if >= 0, is never started) that open the segment (PREFIX, ID) and run one round
// per N_r.  Rank k contributes (+1e16, 1.0, -1e16)[k % 3] * (1 + i + r) at index i of round r: a sum whose bits depend on
// the order of the ranks.  Every rank reports, per round, one line
//   rank K round R seq S ok HEX      HEX: the n results, each as the 16 hex digits of its bit pattern
//   rank K round R seq S err size    hx_begin refused the length
//   rank K round R seq S err rank J  rank J did not answer (the rank stops there)
// and rank 0 a first line "name /NAME".  Exit status 0 when every started rank exited with 0.
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>

#include <string>
#include <vector>

#include "host_exchange.h"

static std::string run_rank(const char* prefix, const char* id, int rank, int world, HxWait wait, int cap, double timeout_s,
                            const std::vector<long long>& ns) {
    std::string out;
    char line[128];
    HostExchange* c = hx_open(prefix, id, (int)strlen(id), rank, world, cap, wait, timeout_s);
    if (!c) return "rank " + std::to_string(rank) + " open failed\n";
    if (rank == 0) out += std::string("name ") + c->name + "\n";
    const double pattern[3] = {1e16, 1.0, -1e16};
    for (size_t r = 0; r < ns.size(); ++r) {
        const long long n = ns[r];
        std::vector<double> res((size_t)(n > 0 ? n : 0));
        double* mine = nullptr;
        int rc = hx_begin(c, n, &mine);
        if (rc == HX_OK) {
            for (long long i = 0; i < n; ++i) mine[i] = pattern[rank % 3] * (double)(1 + i + (long long)r);
            rc = hx_finish(c, res.data());
        }
        snprintf(line, sizeof(line), "rank %d round %zu seq %lld ", rank, r, c->seq);
        out += line;
        if (rc == HX_ERR_SIZE) out += "err size\n";
        else if (rc == HX_ERR_RANK) out += "err rank " + std::to_string(c->silent) + "\n";
        else {
            out += "ok ";
            for (double v : res) {
                unsigned long long bits;
                memcpy(&bits, &v, sizeof(bits));
                snprintf(line, sizeof(line), "%016llx", bits);
                out += line;
            }
            out += "\n";
        }
        if (rc == HX_ERR_RANK) break;
    }
    hx_close(c);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 9) {
        fprintf(stderr, "usage: %s PREFIX ID WORLD sleep|spin CAP TIMEOUT_S MISSING N_0 [N_1 ...]\n", argv[0]);
        return 2;
    }
    const char *prefix = argv[1], *id = argv[2];
    const int world = atoi(argv[3]), cap = atoi(argv[5]), missing = atoi(argv[7]);
    const HxWait wait = strcmp(argv[4], "spin") == 0 ? HX_SPIN : HX_SLEEP;
    const double timeout_s = atof(argv[6]);
    std::vector<long long> ns;
    for (int i = 8; i < argc; ++i) ns.push_back(atoll(argv[i]));
    if (world < 1 || world > 64) return 2;

    // every rank keeps its report until its rounds are over, then writes it into a pipe of its own: nobody waits for
    // the parent in the middle of a round
    std::vector<int> fds(world, -1);
    std::vector<pid_t> pids(world, -1);
    for (int k = 0; k < world; ++k) {
        if (k == missing) continue;
        int p[2];
        if (pipe(p) != 0) return 3;
        pids[k] = fork();
        if (pids[k] < 0) return 3;
        if (pids[k] == 0) {
            close(p[0]);
            for (int j = 0; j < k; ++j)
                if (fds[j] >= 0) close(fds[j]);
            const std::string out = run_rank(prefix, id, k, world, wait, cap, timeout_s, ns);
            for (size_t done = 0; done < out.size();) {
                const ssize_t w = write(p[1], out.data() + done, out.size() - done);
                if (w <= 0) return 4;
                done += (size_t)w;
            }
            close(p[1]);
            return 0;
        }
        close(p[1]);
        fds[k] = p[0];
    }
    int status = 0;
    std::vector<char> buf(1 << 16);
    for (int k = 0; k < world; ++k) {
        if (fds[k] < 0) continue;
        for (ssize_t got; (got = read(fds[k], buf.data(), buf.size())) > 0;) fwrite(buf.data(), 1, (size_t)got, stdout);
        close(fds[k]);
        int st = 0;
        if (waitpid(pids[k], &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) {
            fprintf(stderr, "rank %d: wait status %d\n", k, st);
            status = 1;
        }
    }
    return status;
}
