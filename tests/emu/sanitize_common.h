// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// What the sections of the sanitizer driver (tests/emu/sanitize_*.cpp, one binary: see sanitize_main.cpp) share: the error
// checks, a seeded generator and the classical-MENT slot descriptors.  Each section calls seed() on entry, so its synthetic
// inputs do not depend on the sections that ran before it.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mentflow_hip.h"

void sanitize_ment();
void sanitize_mcmc();
void sanitize_entropy();
void sanitize_swd();

#define CK(call)                                                                 \
    do {                                                                         \
        if ((call) != 0) {                                                       \
            fprintf(stderr, "FAILED %s: %s\n", #call, mf_last_error());          \
            exit(2);                                                             \
        }                                                                        \
    } while (0)

static void check(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "check failed: %s\n", what);
        exit(3);
    }
}

static unsigned g_urand_state = 0u;      // one per section (translation unit)
static void seed(unsigned s) { g_urand_state = s; }
static float urand() {                         // [0, 1)
    g_urand_state = g_urand_state * 1664525u + 1013904223u;
    return (float)(g_urand_state >> 8) / 16777216.0f;
}
static float nrand() {                         // roughly normal: a sum of uniforms
    float s = 0.0f;
    for (int i = 0; i < 6; ++i) s += urand();
    return (s - 3.0f) * 1.4142135f;
}

struct Slots {
    std::vector<float> desc;
    std::vector<int32_t> meta;
    std::vector<float> tables;
    int n = 0;
};

// `dims[k]` = 1 or 2 axes, B bins per axis on [-3, 3]: descriptor layout of include/mentflow_hip.h
static Slots make_slots(int d, const std::vector<int>& dims, int B) {
    Slots s;
    const float delta = 6.0f / B;
    for (int nd : dims) {
        float row[2][8] = {};
        for (int a = 0; a < nd; ++a) {
            float norm = 0.0f;
            for (int j = 0; j < d; ++j) {
                row[a][j] = urand() - 0.5f;
                norm += row[a][j] * row[a][j];
            }
            for (int j = 0; j < d; ++j) row[a][j] /= std::sqrt(norm);
        }
        for (int a = 0; a < 2; ++a)
            for (int j = 0; j < 8; ++j) s.desc.push_back(row[a][j]);
        for (int a = 0; a < 2; ++a) {
            s.desc.push_back(-3.0f + 0.5f * delta);
            s.desc.push_back(3.0f - 0.5f * delta);
            s.desc.push_back(1.0f / delta);
        }
        s.desc.push_back(0.0f);
        s.desc.push_back(0.0f);
        const int size = nd == 1 ? B : B * B;
        s.meta.push_back(nd);
        s.meta.push_back(B);
        s.meta.push_back(nd == 1 ? 1 : B);
        s.meta.push_back((int32_t)s.tables.size());
        for (int i = 0; i < size; ++i) s.tables.push_back(urand() < 0.15f ? 0.0f : 2.0f * urand());
        ++s.n;
    }
    if (s.tables.empty()) s.tables.push_back(0.0f);
    return s;
}
