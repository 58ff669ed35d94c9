/*
 * miro_oracle_photon.c -- restatement of the reference's photon map (Jensen's kd-tree, vendored by the
 * reference as PhotonMap.cpp and modified to take a surface normal): store (PhotonMap.cpp:255-289),
 * scale_photon_power (:298-306), balance / balance_segment / median_split (:314-476), locate_photons
 * (:152-243) and irradiance_estimate (:81-145), as called from Scene::traceScene (Scene.cpp:286-299) with
 * max_dist = PHOTON_MAX_DIST = 1e10 and nphotons = PHOTON_SAMPLES = 500 (Miro.h:16-17).
 * TEST INFRASTRUCTURE ONLY (see miro_oracle.h).
 *
 * PARITY: pinned to the reference's own PhotonMap.cpp on every map WITHOUT A TIED MEDIAN (no node with a child has another
 * photon in its subtree with the same pos[plane]): tests/test_photon_reference.py compares tree, found, dist2[0] and the
 * irradiance bit for bit with tests/golden/photon_ref/, which oracle/_ref/photon_ref wrote (the reference's file compiled
 * unchanged, oracle/ref_photon_driver.cpp).  NOT pinned: maps with a tied median, where median_split below selects by
 * (coordinate, address) and the reference's Sedgewick partition does not (measured in DESIGN.md "Oracle").
 *
 * Quirks kept on purpose:
 *   - a node descends only if index < stored/2 - 1 (:160,:357), so the last three heap slots are never visited;
 *   - dist2[0] keeps max_dist^2 until the (k+1)-th candidate arrives (:192-241), so a query that finds
 *     <= k candidates is normalised by max_dist^2;
 *   - the facing test uses the direction quantised to two bytes through the cos/sin tables (:47-53,:66-71).
 */
#include "miro_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

typedef struct {
    float pos[3];
    short plane;
    unsigned char theta, phi;
    float power[3];
} photon;                                              /* PhotonMap.h:16-22, 28 bytes */

struct orc_pmap {
    photon *ph;                                        /* 1-based */
    int stored, half_stored, max, prev_scale;
    float costheta[256], sintheta[256], cosphi[256], sinphi[256];
    float bmin[3], bmax[3];
};

orc_pmap *orc_pmap_new(int max_photons)
{
    orc_pmap *m = (orc_pmap *)calloc(1, sizeof(orc_pmap));
    m->max = max_photons;
    m->prev_scale = 1;
    m->ph = (photon *)calloc((size_t)max_photons + 2, sizeof(photon));
    for (int k = 0; k < 3; k++) { m->bmin[k] = 1e8f; m->bmax[k] = -1e8f; }
    for (int i = 0; i < 256; i++) {                    /* :47-53 */
        double angle = (double)i * (1.0 / 256.0) * M_PI;
        m->costheta[i] = (float)cos(angle);
        m->sintheta[i] = (float)sin(angle);
        m->cosphi[i] = (float)cos(2.0 * angle);
        m->sinphi[i] = (float)sin(2.0 * angle);
    }
    return m;
}

void orc_pmap_free(orc_pmap *m) { if (m) { free(m->ph); free(m); } }

int orc_pmap_count(const orc_pmap *m) { return m->stored; }

/* Photon_map::store, n photons at once */
void orc_pmap_store(orc_pmap *m, int n, const float *power, const float *pos, const float *dir)
{
    for (int i = 0; i < n; i++) {
        if (m->stored >= m->max) return;
        photon *p = &m->ph[++m->stored];
        for (int k = 0; k < 3; k++) {
            p->pos[k] = pos[3 * i + k];
            if (p->pos[k] < m->bmin[k]) m->bmin[k] = p->pos[k];
            if (p->pos[k] > m->bmax[k]) m->bmax[k] = p->pos[k];
            p->power[k] = power[3 * i + k];
        }
        int theta = (int)(acos(dir[3 * i + 2]) * (256.0 / M_PI));
        p->theta = theta > 255 ? 255 : (unsigned char)theta;
        int phi = (int)(atan2(dir[3 * i + 1], dir[3 * i]) * (256.0 / (2.0 * M_PI)));
        if (phi > 255) p->phi = 255;
        else if (phi < 0) p->phi = (unsigned char)(phi + 256);
        else p->phi = (unsigned char)phi;
    }
}

void orc_pmap_scale(orc_pmap *m, float scale)
{
    for (int i = m->prev_scale; i <= m->stored; i++)
        for (int k = 0; k < 3; k++) m->ph[i].power[k] *= scale;
    m->prev_scale = m->stored;
}

/* median_split (:375-404) places the photon of rank `median` (by pos[axis]) at porg[median], smaller ones before
 * it, larger ones after it.  Restated as a plain quick-select with a total order (coordinate, then address) so that
 * the resulting tree is unique even when coordinates repeat; with distinct coordinates any selection algorithm
 * -- the reference's included -- yields the same left / right sets and therefore the same tree. */
static inline int before(const photon *a, const photon *b, int axis)
{
    if (a->pos[axis] != b->pos[axis]) return a->pos[axis] < b->pos[axis];
    return a < b;
}
static void median_split(photon **p, int start, int end, int median, int axis)
{
    int lo = start, hi = end;
    while (lo < hi) {
        photon *pivot = p[lo + (hi - lo) / 2];
        int i = lo, j = hi;
        while (i <= j) {
            while (before(p[i], pivot, axis)) i++;
            while (before(pivot, p[j], axis)) j--;
            if (i <= j) { photon *t = p[i]; p[i] = p[j]; p[j] = t; i++; j--; }
        }
        if (median <= j) hi = j;
        else if (median >= i) lo = i;
        else return;
    }
}

/* balance_segment (:409-476) */
static void balance_segment(orc_pmap *m, photon **pbal, photon **porg, int index, int start, int end)
{
    int median = 1;
    while ((4 * median) <= (end - start + 1)) median += median;
    if ((3 * median) <= (end - start + 1)) { median += median; median += start - 1; }
    else median = end - median + 1;

    int axis = 2;
    if ((m->bmax[0] - m->bmin[0]) > (m->bmax[1] - m->bmin[1]) && (m->bmax[0] - m->bmin[0]) > (m->bmax[2] - m->bmin[2])) axis = 0;
    else if ((m->bmax[1] - m->bmin[1]) > (m->bmax[2] - m->bmin[2])) axis = 1;

    median_split(porg, start, end, median, axis);
    pbal[index] = porg[median];
    pbal[index]->plane = (short)axis;

    if (median > start) {
        if (start < median - 1) {
            const float tmp = m->bmax[axis];
            m->bmax[axis] = pbal[index]->pos[axis];
            balance_segment(m, pbal, porg, 2 * index, start, median - 1);
            m->bmax[axis] = tmp;
        } else pbal[2 * index] = porg[start];
    }
    if (median < end) {
        if (median + 1 < end) {
            const float tmp = m->bmin[axis];
            m->bmin[axis] = pbal[index]->pos[axis];
            balance_segment(m, pbal, porg, 2 * index + 1, median + 1, end);
            m->bmin[axis] = tmp;
        } else pbal[2 * index + 1] = porg[end];
    }
}

/* Photon_map::balance (:314-359): heap-ordered copy instead of the in-place cycle walk (same result) */
void orc_pmap_balance(orc_pmap *m)
{
    if (m->stored > 1) {
        photon **pa1 = (photon **)calloc((size_t)m->stored + 2, sizeof(photon *));
        photon **pa2 = (photon **)calloc((size_t)m->stored + 2, sizeof(photon *));
        for (int i = 0; i <= m->stored; i++) pa2[i] = &m->ph[i];
        balance_segment(m, pa1, pa2, 1, 1, m->stored);
        photon *out = (photon *)calloc((size_t)m->max + 2, sizeof(photon));
        for (int i = 1; i <= m->stored; i++) out[i] = *pa1[i];
        free(m->ph);
        m->ph = out;
        free(pa1); free(pa2);
    }
    m->half_stored = m->stored / 2 - 1;
}

/* the k-nearest candidate set of locate_photons: slots 1..found; slot 0 of dist2 is the pruning radius^2 */
typedef struct {
    int max, found, heaped;
    float pos[3];
    float *dist2;
    int *index;
} nearest;

static inline void photon_dir(const orc_pmap *m, const photon *p, float *d)
{
    d[0] = m->sintheta[p->theta] * m->cosphi[p->phi];            /* :66-71 */
    d[1] = m->sintheta[p->theta] * m->sinphi[p->phi];
    d[2] = m->costheta[p->theta];
}

/* max-heap on dist2[1..n]: move the hole at `at` down until (d, id) fits.  The reference stops at a child of the SAME distance
 * while it builds the heap (:210, `>=`) and passes it while it inserts (:230, `>`): with equal distances in the heap that decides
 * which photon sits at the root, and with it which of them the next insertion drops. */
static void sift_down(nearest *np, int at, float d, int id, int pass_equal)
{
    const int n = np->found;
    for (;;) {
        int c = 2 * at;
        if (c > n) break;
        if (c < n && np->dist2[c] < np->dist2[c + 1]) c++;
        if (pass_equal ? d > np->dist2[c] : d >= np->dist2[c]) break;
        np->dist2[at] = np->dist2[c];
        np->index[at] = np->index[c];
        at = c;
    }
    np->dist2[at] = d;
    np->index[at] = id;
}

/* :186-241 -- a photon that passed the distance and facing tests */
static void offer(nearest *np, float d, int id)
{
    if (np->found < np->max) {                       /* :189-193: plain array while there is room */
        np->found++;
        np->dist2[np->found] = d;
        np->index[np->found] = id;
        return;
    }
    if (!np->heaped) {                               /* :197-217: heapify once, on the first overflow */
        for (int k = np->found >> 1; k >= 1; k--) sift_down(np, k, np->dist2[k], np->index[k], 0);
        np->heaped = 1;
    }
    sift_down(np, 1, d, id, 1);                       /* :222-238: replace the farthest */
    np->dist2[0] = np->dist2[1];                     /* :240: the radius shrinks only from now on */
}

/* locate_photons (:152-243): near side first, far side only if the plane is closer than the current radius;
 * the node itself is examined after its subtrees */
static void locate(const orc_pmap *m, nearest *np, int index, const float *normal)
{
    const photon *p = &m->ph[index];
    if (index < m->half_stored) {                    /* :160 */
        const float side = np->pos[p->plane] - p->pos[p->plane];
        const int near_child = side > 0.0 ? 2 * index + 1 : 2 * index;
        locate(m, np, near_child, normal);
        if (side * side < np->dist2[0]) locate(m, np, near_child ^ 1, normal);
    }
    float dx = p->pos[0] - np->pos[0];
    float d = dx * dx;
    dx = p->pos[1] - np->pos[1];
    d += dx * dx;
    dx = p->pos[2] - np->pos[2];
    d += dx * dx;
    float pdir[3];
    photon_dir(m, p, pdir);
    if (d < np->dist2[0] && (pdir[0] * normal[0] + pdir[1] * normal[1] + pdir[2] * normal[2]) < 0.0f)
        offer(np, d, index);
}

/* irradiance_estimate (:81-145) for nq queries; found / r2 are optional diagnostics (np.found, np.dist2[0]) */
void orc_pmap_irradiance(const orc_pmap *m, uint64_t nq, const float *pos, const float *normal, float max_dist,
                         int nphotons, float *irrad, int *found, float *r2)
{
    float *d2 = (float *)malloc(sizeof(float) * (size_t)(nphotons + 1));
    int *idx = (int *)malloc(sizeof(int) * (size_t)(nphotons + 1));
    for (uint64_t q = 0; q < nq; q++) {
        float ir[3] = {0.0f, 0.0f, 0.0f};
        nearest np;
        np.dist2 = d2; np.index = idx;
        np.pos[0] = pos[3 * q]; np.pos[1] = pos[3 * q + 1]; np.pos[2] = pos[3 * q + 2];
        np.max = nphotons; np.found = 0; np.heaped = 0;
        np.dist2[0] = max_dist * max_dist;
        if (m->stored > 0) locate(m, &np, 1, &normal[3 * q]);
        for (int i = 1; i <= np.found; i++) {
            const photon *p = &m->ph[np.index[i]];
            ir[0] += p->power[0]; ir[1] += p->power[1]; ir[2] += p->power[2];
        }
        const float tmp = (float)((1.0f / M_PI) / (np.dist2[0]));
        irrad[3 * q] = ir[0] * tmp; irrad[3 * q + 1] = ir[1] * tmp; irrad[3 * q + 2] = ir[2] * tmp;
        if (found) found[q] = np.found;
        if (r2) r2[q] = np.dist2[0];
    }
    free(d2); free(idx);
}

/* brute force over the *reachable* heap slots with the same candidate rule (self-consistency check) */
void orc_pmap_irradiance_brute(const orc_pmap *m, uint64_t nq, const float *pos, const float *normal, float max_dist,
                               int nphotons, float *irrad, int *found, float *r2)
{
    /* reachable: root, and children of any node with index < half_stored */
    float *cand = (float *)malloc(sizeof(float) * (size_t)(m->stored + 2));
    int *cidx = (int *)malloc(sizeof(int) * (size_t)(m->stored + 2));
    for (uint64_t q = 0; q < nq; q++) {
        int nc = 0;
        const float md2 = max_dist * max_dist;
        for (int i = 1; i <= m->stored; i++) {
            if (i > 1 && !((i >> 1) < m->half_stored)) continue;
            const photon *p = &m->ph[i];
            float d1 = p->pos[0] - pos[3 * q], dd = d1 * d1;
            d1 = p->pos[1] - pos[3 * q + 1]; dd += d1 * d1;
            d1 = p->pos[2] - pos[3 * q + 2]; dd += d1 * d1;
            float pd[3];
            photon_dir(m, p, pd);
            if (dd < md2 && (pd[0] * normal[3 * q] + pd[1] * normal[3 * q + 1] + pd[2] * normal[3 * q + 2]) < 0.0f) { cand[nc] = dd; cidx[nc++] = i; }
        }
        /* partial selection sort of the k smallest */
        int k = nc < nphotons ? nc : nphotons;
        for (int a = 0; a < k; a++) {
            int best = a;
            for (int b = a + 1; b < nc; b++) if (cand[b] < cand[best]) best = b;
            float t = cand[a]; cand[a] = cand[best]; cand[best] = t;
            int ti = cidx[a]; cidx[a] = cidx[best]; cidx[best] = ti;
        }
        double ir[3] = {0, 0, 0};
        for (int a = 0; a < k; a++) for (int c = 0; c < 3; c++) ir[c] += m->ph[cidx[a]].power[c];
        const float rr = nc > nphotons ? cand[k - 1] : md2;
        const float tmp = (float)((1.0f / M_PI) / rr);
        for (int c = 0; c < 3; c++) irrad[3 * q + c] = (float)ir[c] * tmp;
        if (found) found[q] = k;
        if (r2) r2[q] = rr;
    }
    free(cand); free(cidx);
}

/* heap-ordered export for comparison with the product's balance: pos[3n], plane[n], theta/phi as dir bytes, power[3n] */
void orc_pmap_export(const orc_pmap *m, float *pos, int *plane, unsigned char *theta_phi, float *power)
{
    for (int i = 1; i <= m->stored; i++) {
        for (int k = 0; k < 3; k++) { pos[3 * (i - 1) + k] = m->ph[i].pos[k]; power[3 * (i - 1) + k] = m->ph[i].power[k]; }
        plane[i - 1] = m->ph[i].plane;
        theta_phi[2 * (i - 1)] = m->ph[i].theta;
        theta_phi[2 * (i - 1) + 1] = m->ph[i].phi;
    }
}
