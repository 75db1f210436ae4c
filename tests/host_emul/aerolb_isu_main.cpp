// TEST INFRASTRUCTURE ONLY: a program of its own around aerolb_isu_emul.cpp, for a run under the address and undefined-behaviour sanitizers
// (tests/test_aerolb_isu_sanitize.py builds it with g++ -fsanitize=address,undefined and runs it; nothing is loaded into Python).
//   aerolb_isu_main <fb> <msg_cap> <width> <streams file>
// The file: int32 nch, then per channel int32 n and n int16 soft entries.  The streams are written in ragged per-channel pieces of at most
// `width` entries, as the tests do; per channel one line goes to stdout: channel, messages in the log, overflow word, the eight counters.
#include <cstdio>
#include <cstdlib>

#include "aerolb_isu_emul.cpp"

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s fb msg_cap width streams\n", argv[0]); return 2; }
    const int fb = atoi(argv[1]), msg_cap = atoi(argv[2]), width = atoi(argv[3]);
    FILE *f = fopen(argv[4], "rb");
    if (!f) { perror(argv[4]); return 2; }
    int32_t nch = 0;
    if (fread(&nch, 4, 1, f) != 1 || nch < 1 || width < 1 || msg_cap < 1) return 2;
    std::vector<std::vector<int16_t>> s((size_t)nch);
    for (auto &x : s)
    {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
        x.resize((size_t)n);
        if (n && fread(x.data(), 2, (size_t)n, f) != (size_t)n) return 2;
    }
    fclose(f);
    EmulR *x = emulr_create(nch, fb, 700, msg_cap);
    // exactly nch rows of `width` entries: a walk past a row's count, or the wide path past a row's end, is the sanitizer's to find
    int16_t *buf = nullptr;
    if (posix_memalign((void **)&buf, 16, (size_t)nch * width * sizeof(int16_t))) return 2;
    std::vector<int> cnt((size_t)nch);
    std::vector<size_t> pos((size_t)nch, 0);
    unsigned lcg = 12345u + (unsigned)fb;
    for (bool more = true; more;)
    {
        more = false;
        int mx = 0;
        memset(buf, 0, (size_t)nch * width * sizeof(int16_t));
        for (int c = 0; c < nch; c++)
        {
            lcg = lcg * 1664525u + 1013904223u;
            size_t n = 1 + (lcg >> 8) % (unsigned)width;
            if (n > s[c].size() - pos[c]) n = s[c].size() - pos[c];
            if (n) memcpy(buf + (size_t)c * width, s[c].data() + pos[c], n * sizeof(int16_t));
            pos[c] += n;
            cnt[c] = (int)n;
            if ((int)n > mx) mx = (int)n;
            if (pos[c] < s[c].size()) more = true;
        }
        if (emulr_write(x, buf, cnt.data(), width, mx)) return 3;
    }
    for (int c = 0; c < nch; c++)
    {
        long long st[RT_NSTATS];
        emulr_stats(x, c, st);
        printf("%d %d %d", c, x->q.msg_cnt[c], emulr_overflow(x, c));
        for (int k = 0; k < RT_NSTATS; k++) printf(" %lld", st[k]);
        printf("\n");
    }
    free(buf);
    emulr_destroy(x);
    return 0;
}
