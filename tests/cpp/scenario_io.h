// scenario_io.h -- the readers of the drivers' scenario.txt files: a float as the hex of its bits, a double as the hex of its, an integer in decimal.
#pragma once
#include <cstdio>
#include <cstring>
#include <stdexcept>
static inline float rdf(FILE *f) { unsigned u = 0; if (fscanf(f, "%x", &u) != 1) throw std::runtime_error("scenario: float"); float v; memcpy(&v, &u, 4); return v; }
static inline double rdd(FILE *f) { unsigned long long u = 0; if (fscanf(f, "%llx", &u) != 1) throw std::runtime_error("scenario: double"); double v; memcpy(&v, &u, 8); return v; }
static inline long long rdi(FILE *f) { long long v = 0; if (fscanf(f, "%lld", &v) != 1) throw std::runtime_error("scenario: int"); return v; }
