/*
 * ref_photon_driver.cpp -- runs the reference's own Photon_map (its PhotonMap.cpp, compiled unchanged next to this file by
 * `make ref`) on one job file and writes what it computed to one result file.  TEST INFRASTRUCTURE ONLY: the fixtures under
 * tests/golden/photon_ref/ are this program's output (tests/golden/make_photon_ref.py); the product never sees it.
 *
 * Built with -fno-access-control so that photons, stored_photons and half_stored_photons can be read as they are.
 * Photon_map::balance prints to stdout, so results go to a file.  Everything is little-endian, 4-byte aligned:
 *
 *   job:     "PMJ1"  capacity:i32  n_batches:i32  n_groups:i32
 *            per batch:  n:i32  scale:f32  power[3n]:f32  pos[3n]:f32  dir[3n]:f32
 *            per group:  k:i32  max_dist:f32  nq:i32  pos[3nq]:f32  normal[3nq]:f32
 *            replayed as store x n, scale_photon_power(scale) per batch in order, then balance(), then the groups.
 *
 *   result:  "PMR1"  stored:i32  half_stored:i32  n_groups:i32
 *            pos[3*stored]:f32  power[3*stored]:f32  plane[stored]:i32  theta_phi[2*stored]:u8 (padded to 4)  origin[stored]:i32
 *              in heap order, slot 1 first.  plane is -1 where 2*i > stored: balance_segment never writes a leaf's plane and
 *              store() does not initialise it.  origin is the 0-based rank, among the photons that were stored, of the photon in
 *              that slot; it comes from a second Photon_map given the same positions with that rank as power[0] -- balance()
 *              looks at nothing but positions and the box, so both maps balance alike, which is verified slot by slot.
 *            per group:  found[nq]:i32  dist2_0[nq]:f32  irradiance[3nq]:f32  candidates[nq*k]:i32
 *              found, dist2[0] and candidates (heap slots np.index[1..found] in the array's own order, 0 beyond found) are from a
 *              direct locate_photons call set up as irradiance_estimate sets it up; irradiance is irradiance_estimate's.  The
 *              driver checks that summing the candidates' powers in that order reproduces irradiance_estimate bit for bit.
 *
 * An empty map is not queried: locate_photons(np, 1, ...) would read photons[1], which nothing has written.  A job with
 * stored == 0 and query groups is refused.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "PhotonMap.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

static void die(const char *what)
{
    fprintf(stderr, "ref_photon_driver: %s\n", what);
    exit(2);
}

template <typename T> static void get(FILE *f, T *dst, size_t n)
{
    if (n && fread(dst, sizeof(T), n, f) != n) die("job file too short");
}

template <typename T> static void put(FILE *f, const T *src, size_t n)
{
    if (n && fwrite(src, sizeof(T), n, f) != n) die("cannot write the result");
}

struct Batch {
    int n;
    float scale;
    std::vector<float> power, pos, dir;
};

struct Group {
    int k, nq;
    float max_dist;
    std::vector<float> pos, normal;
};

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: photon_ref JOB RESULT");
    FILE *in = fopen(argv[1], "rb");
    if (!in) die("cannot open the job");
    char magic[4];
    int32_t head[3];
    get(in, magic, 4);
    if (memcmp(magic, "PMJ1", 4) != 0) die("not a job file");
    get(in, head, 3);
    const int capacity = head[0], n_batches = head[1], n_groups = head[2];
    if (capacity < 1 || n_batches < 0 || n_groups < 0) die("bad header");

    std::vector<Batch> batches(n_batches);
    for (Batch &b : batches) {
        get(in, &b.n, 1);
        get(in, &b.scale, 1);
        if (b.n < 0) die("bad batch");
        b.power.resize(3 * (size_t)b.n); b.pos.resize(3 * (size_t)b.n); b.dir.resize(3 * (size_t)b.n);
        get(in, b.power.data(), b.power.size());
        get(in, b.pos.data(), b.pos.size());
        get(in, b.dir.data(), b.dir.size());
    }
    std::vector<Group> groups(n_groups);
    for (Group &g : groups) {
        get(in, &g.k, 1);
        get(in, &g.max_dist, 1);
        get(in, &g.nq, 1);
        if (g.k < 1 || g.nq < 0) die("bad group");
        g.pos.resize(3 * (size_t)g.nq); g.normal.resize(3 * (size_t)g.nq);
        get(in, g.pos.data(), g.pos.size());
        get(in, g.normal.data(), g.normal.size());
    }
    fclose(in);

    /* the map under test, and its shadow whose power[0] names the photon */
    Photon_map map(capacity), shadow(capacity);
    int rank = 0;
    for (const Batch &b : batches) {
        for (int i = 0; i < b.n; i++) {
            map.store(&b.power[3 * i], &b.pos[3 * i], &b.dir[3 * i]);
            const float tag[3] = {(float)rank, 0.0f, 0.0f};
            shadow.store(tag, &b.pos[3 * i], &b.dir[3 * i]);
            rank++;
        }
        map.scale_photon_power(b.scale);
    }
    if (rank > (1 << 24)) die("too many photons to tag in a float");
    map.balance();
    shadow.balance();

    const int stored = map.stored_photons;
    if (shadow.stored_photons != stored) die("the shadow map stored a different number");
    if (stored == 0 && n_groups > 0) die("an empty map is not queried (locate_photons would read an unwritten photon)");

    FILE *out = fopen(argv[2], "wb");
    if (!out) die("cannot open the result");
    const int32_t rhead[3] = {stored, map.half_stored_photons, n_groups};
    put(out, "PMR1", 4);
    put(out, rhead, 3);

    std::vector<float> pos(3 * (size_t)stored), power(3 * (size_t)stored);
    std::vector<int32_t> plane(stored), origin(stored);
    std::vector<unsigned char> tp((2 * (size_t)stored + 3) / 4 * 4, 0);
    for (int i = 1; i <= stored; i++) {
        const Photon &p = map.photons[i], &s = shadow.photons[i];
        if (memcmp(p.pos, s.pos, sizeof p.pos) != 0 || p.theta != s.theta || p.phi != s.phi) die("the shadow map balanced differently");
        const bool has_child = 2 * i <= stored;
        if (has_child && p.plane != s.plane) die("the shadow map split differently");
        for (int c = 0; c < 3; c++) { pos[3 * (i - 1) + c] = p.pos[c]; power[3 * (i - 1) + c] = p.power[c]; }
        plane[i - 1] = has_child ? p.plane : -1;
        tp[2 * (i - 1)] = p.theta;
        tp[2 * (i - 1) + 1] = p.phi;
        origin[i - 1] = (int32_t)s.power[0];
        if (origin[i - 1] < 0 || origin[i - 1] >= stored || (float)origin[i - 1] != s.power[0]) die("bad tag");
    }
    put(out, pos.data(), pos.size());
    put(out, power.data(), power.size());
    put(out, plane.data(), plane.size());
    put(out, tp.data(), tp.size());
    put(out, origin.data(), origin.size());

    for (const Group &g : groups) {
        std::vector<int32_t> found(g.nq), cand((size_t)g.nq * g.k, 0);
        std::vector<float> r2(g.nq), irr(3 * (size_t)g.nq);
        std::vector<float> d2(g.k + 1);
        std::vector<const Photon *> idx(g.k + 1);
        for (int q = 0; q < g.nq; q++) {
            const float *qp = &g.pos[3 * q], *qn = &g.normal[3 * q];
            NearestPhotons np;
            np.dist2 = d2.data();
            np.index = idx.data();
            np.pos[0] = qp[0]; np.pos[1] = qp[1]; np.pos[2] = qp[2];
            np.max = g.k;
            np.found = 0;
            np.got_heap = 0;
            np.dist2[0] = g.max_dist * g.max_dist;
            map.locate_photons(&np, 1, qn);
            found[q] = np.found;
            r2[q] = np.dist2[0];
            float sum[3] = {0.0f, 0.0f, 0.0f};
            for (int i = 1; i <= np.found; i++) {
                const long slot = np.index[i] - map.photons;
                if (slot < 1 || slot > stored) die("a candidate outside the heap");
                cand[(size_t)q * g.k + (i - 1)] = (int32_t)slot;
                sum[0] += np.index[i]->power[0]; sum[1] += np.index[i]->power[1]; sum[2] += np.index[i]->power[2];
            }
            map.irradiance_estimate(&irr[3 * q], qp, qn, g.max_dist, g.k);
            const float tmp = (1.0f / M_PI) / (np.dist2[0]);
            for (int c = 0; c < 3; c++) {
                const float mine = sum[c] * tmp;
                if (memcmp(&mine, &irr[3 * q + c], sizeof mine) != 0) die("irradiance_estimate is not the sum over the candidates");
            }
        }
        put(out, found.data(), found.size());
        put(out, r2.data(), r2.size());
        put(out, irr.data(), irr.size());
        put(out, cand.data(), cand.size());
    }
    if (fclose(out) != 0) die("cannot close the result");
    return 0;
}
