// pt_shade_visit.h — logicSlot: one visit of the path tracer to one slot (gfx950, wave64): resolve the pending next-event estimate,
// shade the hit that came back (getSurfacePoint, emission + MIS, Russian roulette), then the next bounce: light sampling + BSDF
// sampling (Renderers/PathTracingRenderer.cpp:137-262).  k_shade (pt_shade_kernels.h) and the tail kernel (pt_tail_kernels.h) both
// call it.
#pragma once
#include "pt_bsdf.h"
#include "pt_bsdf_multi.h"
#include "pt_env_sphere.h"
#include "pt_kernels.h"
#include "pt_shade_tables.h"
#include "pt_slot_state.h"
#include "pt_surface.h"
#include "pt_tex.h"
#include "pt_tex_spectrum.h"

namespace slrhip {

// One visit of the shade kernel to one slot: everything between the state loads and the state stores.  A device function so
// that the tail kernel (pt_tail_kernels.h) runs the very same code on the last paths of a render call.
// FUSED (k_shade): a path that ends here is accumulated and restarted by the caller in the same launch — the slot's flags and
// radiance sum are handed back (`flags`, `radiance`; RGB keeps the sum in registers) instead of being stored.  Not FUSED
// (k_tail): the slot is left in ST_REGEN with bit 15 set and its sum in HBM, for the lane's next turn.
// TIGHT (k_shade's fused start without the glossy lobes): the visit holds no address of a state record from its loads
// to its stores.  The same instructions on the same values; set only where the 14 registers decide a wave per SIMD.
template <class S, bool LDS_TABLES, bool MF, bool MULTI, bool TEX, bool FUSED, bool TIGHT = false>
__device__ __forceinline__ void logicSlot(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, const ShadeLds<S::N != 3>& lds,
                                          const float* lightPMF, const float* lightCDF, uint32_t slot, const SlotLoads<S>& in, uint32_t& flags, uint32_t vis,
                                          S& radiance, bool& emitExt, bool& emitShadow, bool& emitRegen, bool* deadShadow = nullptr) {
    // Light samples that decide nothing are not traced (step 3): k_shade's RGB kernels, whose Kahan pair is in registers.
    // The spectral kernels (the pair is in HBM) and k_tail (it traces its shadow ray inline) keep their code.
    constexpr bool kSkipDead = S::N == 3 && FUSED;
    // ---- the state loads that depend on the flags; the others were requested by the caller (SlotLoads) -----------
    const uint4 r4 = in.r4;
    // The path's radiance sum (Kahan pair) and the pending light sample: RGB keeps them in registers (3 x 16 B,
    // requested with everything else); in spectral mode they are 3 x 64 B that most visits never touch, so they
    // stay in HBM and SpAcc updates them in place when a contribution actually arrives.
    S alpha = in.alpha;
    SpAcc<S> sp;
    float bsdfPDFprev = in.pdfPrev;
    sp.begin(pb, slot, rp.numSlots, flags, F_SHADOW(flags) && vis);
    const float4 h = in.h;
    const int32_t hitInstance = in.hitInstance;
    const float4 o4 = in.o4, d4 = in.d4;
    const float wlOffset = in.wlOffset;

    const uint32_t state = F_STATE(flags);
    if (state == ST_FIRST_HIT || state == ST_NEXT_HIT || state == ST_FINISH) {
        // a path's first visit: throughput 1, no previous PDF, empty radiance sum (startSample writes none of them)
        if (state == ST_FIRST_HIT) { alpha = S(1.0f); bsdfPDFprev = 0.0f; }
        sp.startPath(state == ST_FIRST_HIT, flags);
        Rng rng;
        rng.s0 = r4.x; rng.s1 = r4.y; rng.s2 = r4.z; rng.s3 = r4.w;
        uint32_t pathLength = F_PATHLEN(flags), wlSel = F_WLSEL(flags);
        const uint32_t wl = F_WL(flags);
        V3 rayOrg(o4.x, o4.y, o4.z), rayDir(d4.x, d4.y, d4.z);
        float rayTmin = 0.0f;
        SurfPt surf;
        V3 dirOut_sn;
        bool haveSurf = false;
        bool finish = false;
        const uint32_t tri = __float_as_uint(h.x);

        // the hit triangle's shading record: issued before anything else is computed
        float4 q0, q1, q2, q3, q4, q5;
        const bool hasHit = state != ST_FINISH && tri != 0xFFFFFFFFu;
        if (hasHit) {
            const float4* st = reinterpret_cast<const float4*>(sc.shadeTris) + (size_t)tri * 6;
            q0 = st[0]; q1 = st[1]; q2 = st[2]; q3 = st[3]; q4 = st[4]; q5 = st[5];
        }

        // ---- 1. resolve the pending next-event estimate (:180,202) ---------------------------------
        if (F_SHADOW(flags) && vis) sp.addPendingNee(pb, slot, rp.numSlots);      // (its operands were requested with the state loads: SpAcc::begin)

        // ---- 2. the hit that just came back ------------------------------------------------------------
        Mat<S> m;
        float texU = 0.0f, texV = 0.0f;
        int32_t normalMap = -1;
        const auto texturize = [&](Mat<S>& mm, uint32_t matIndex) -> int32_t { return texturizeMat<S>(sc, mm, matIndex, texU, texV, wlOffset); };
        if (!hasHit) {
            finish = true;                      // ST_FINISH, or a miss: :148 return Zero / :226 break
            if (state != ST_FINISH && sc.hasEnv) {
                // the ray left the scene: Scene::intersect falls through to the environment sphere (SurfaceObject.cpp:411-414).
                // InfiniteSphere::intersect / getSurfacePoint (Surface/InfiniteSphere.cpp:34-59), Vector3::toPolarYUp (Vector3.h:72-75)
                float theta = slrAcos(fminf(1.0f, fmaxf(-1.0f, rayDir.y)));
                float phi = fmodf((float)((double)slrAtan2(-rayDir.x, rayDir.z) + 2 * kPi), (float)(2 * kPi));
                float texU = (float)((double)phi / (2 * kPi)), texV = (float)((double)theta / kPi);
                // emittance x IBLEDF::evaluate = 1 / pi (EDFs/IBLEDF.cpp:19-23)
                S Le = envEmittanceS<S>(sc, texU, texV, wlOffset) * S((float)(1.0 / kPi));
                if (state == ST_FIRST_HIT) {
                    sp.add(pb, slot, rp.numSlots, alpha * Le);             // :152-157, atInfinity -> return sp
                }
                else {
                    // implicit light sampling :232-250; the path ends at infinity before Russian roulette
                    float sumImps = sc.aggImportance + 1.0f;
                    float lightProb = 1.0f / sumImps;                        // Scene::evaluateProb SurfaceObject.cpp:456-457
                    V3 gN = -rayDir;
                    float lightPDF = lightProb * envAreaPDF(sc, phi, theta) * 1.0f / absDot(rayDir, gN);
                    float MISWeight = 1.0f;
                    if (!F_DELTA(flags))
                        MISWeight = (bsdfPDFprev * bsdfPDFprev) / (lightPDF * lightPDF + bsdfPDFprev * bsdfPDFprev);
                    sp.add(pb, slot, rp.numSlots, alpha * Le * MISWeight);
                }
            }
        }
        else {
            // Triangle::getSurfacePoint, Surface/TriangleMesh.cpp:180-215.  isect.p = org + dir * t (:170) — of the ray the triangle
            // was tested with: inside an instance that is the LOCAL ray, invert(sampledTF) * ray (SurfaceObject.cpp:307-311), and the
            // whole surface point is taken to world space at the end (TransformedSurfaceObject::getSurfacePoint, below)
            const float* instMats = hitInstance >= 0 ? reinterpret_cast<const float*>(sc.instances + (size_t)hitInstance * 9u) : nullptr;
            if (instMats) surf.p = mulPoint(instMats + 16, rayOrg) + mulVector(instMats + 16, rayDir) * h.y;
            else surf.p = rayOrg + rayDir * h.y;
            surf.gNormal = V3(q3.w, q4.w, q5.w);
            surf.material = __float_as_uint(q0.w);
            surf.light = (int32_t)__float_as_uint(q1.w);
            surf.areaPDF = q2.w;
            m = MatIO<S>::template load<LDS_TABLES>(sc, lds.mats, surf.material, wlOffset);
            // the hit record carries Moller-Trumbore's (b1, b2)
            const float b1 = h.z, b2hit = h.w;
            if constexpr (TEX) {
                // texCoord from the original barycentrics (TriangleMesh.cpp:160-161), then the textures of this material
                const float4 uvA = sc.triUV[(size_t)tri * 2], uvB = sc.triUV[(size_t)tri * 2 + 1];
                hitTexCoord(uvA, uvB, b1, b2hit, &texU, &texV);
                if (m.type & kMatTexturedBit) normalMap = texturize(m, surf.material);
            }
            surf.frame = triangleShadingFrame(q0, q1, q2, q3, q4, q5, b1, b2hit);
            if constexpr (TEX) {
                if (normalMap >= 0) bumpShadingFrame(sc.textures, (uint32_t)normalMap, texU, texV, surf.frame);
            }
            if (instMats) instanceSurfaceToWorld(instMats, surf);
            haveSurf = true;
            dirOut_sn = surf.frame.toLocal(-rayDir);
            if (surf.light >= 0) {
                S Le = MatIO<S>::template emittance<LDS_TABLES>(sc, lds.mats, surf.material, wlOffset) * S(diffuseEDF(dirOut_sn));
                if (state == ST_FIRST_HIT) {
                    sp.add(pb, slot, rp.numSlots, alpha * Le);             // :152-156
                }
                else {
                    // implicit light sampling with MIS :232-249
                    float lightProb = lightPMF[surf.light] * 1.0f;          // SurfaceObject.cpp:295-298, :78-80
                    if (sc.hasEnv) lightProb = sc.aggImportance / (sc.aggImportance + 1.0f) * lightProb;   // Scene::evaluateProb :459
                    float dist2 = sqLength(rayOrg - surf.p);
                    float lightPDF = lightProb * surf.areaPDF * dist2 / absDot(rayDir, surf.gNormal);
                    float MISWeight = 1.0f;
                    if (!F_DELTA(flags))
                        MISWeight = (bsdfPDFprev * bsdfPDFprev) / (lightPDF * lightPDF + bsdfPDFprev * bsdfPDFprev);
                    sp.add(pb, slot, rp.numSlots, alpha * Le * MISWeight);
                }
            }
            if (state == ST_NEXT_HIT) {
                // Russian roulette :254-258 (initY = importance(One) evaluated like the reference)
                float initY = importance(S(1.0f), wl);
                float continueProb = fminf(importance(alpha, wl) / initY, 1.0f);
                if (rng.nextFloat() < continueProb) alpha = alpha / continueProb;
                else finish = true;
            }
        }

        // ---- 3. next bounce: NEE + BSDF sampling (:161-221) ----------------------------------------------
        if (!finish && haveSurf) {
            ++pathLength;
            if (pathLength >= 100) {
                finish = true;
            }
            else {
                V3 gNorm_sn = surf.frame.toLocal(surf.gNormal);
                uint32_t type = bsdfType(m.type, wlSel);
                // SLRHIP_MATERIAL_MULTI: a MultiBSDF whose components are fetched from the material table on demand
                const auto loadComponent = [&](uint32_t idx) {
                    Mat<S> cm = MatIO<S>::template load<LDS_TABLES>(sc, lds.mats, idx, wlOffset);
                    if constexpr (TEX) { if (cm.type & kMatTexturedBit) (void)texturize(cm, idx); }
                    return cm;
                };
                const bool isMulti = MULTI && m.type == SLRHIP_MATERIAL_MULTI;
                MultiTree multiTree = {};
                if constexpr (MULTI) {
                    if (isMulti) {
                        multiTree = buildMultiTree<S>(decodeMulti(m), loadComponent);
                        type = multiType(multiTree, wlSel);
                    }
                }
                if (dtMatches(type, DT_WholeSphere | DT_NonDelta)) {
                    // Scene::selectLight, SurfaceObject.cpp:432-450 (+ aggregate :279-286)
                    float lightProb;
                    float uSel = rng.nextFloat();
                    bool pickEnv = false;
                    if (sc.hasEnv) {
                        float sumImps = sc.aggImportance + 1.0f;
                        float su = sumImps * uSel;
                        if (su < sc.aggImportance) uSel = uSel / (sc.aggImportance / sumImps);
                        else pickEnv = true;
                    }
                    float lu0 = rng.nextFloat();
                    float lu1 = rng.nextFloat();
                    V3 lp, lgn;
                    Frame lf;
                    float areaPDF;
                    S M;
                    float shadowTmax;
                    V3 sdir;
                    if (pickEnv) {
                        lightProb = 1.0f * (1.0f / (sc.aggImportance + 1.0f));
                        // InfiniteSphereSurfaceObject::sample, SurfaceObject.cpp:158-185
                        float topPDF, rowPDF;
                        float d1 = sampleContinuous1D(sc.envTopCDF, sc.envTopPDF, sc.envMapHeight, lu1, &topPDF);
                        uint32_t idx1D = min((uint32_t)((float)sc.envMapHeight * d1), sc.envMapHeight - 1);
                        float d0 = sampleContinuous1D(sc.envRowCDF + (size_t)idx1D * (sc.envMapWidth + 1), sc.envRowPDF + (size_t)idx1D * sc.envMapWidth,
                                                      sc.envMapWidth, lu0, &rowPDF);
                        float uvPDF = rowPDF * topPDF;
                        float phi = (float)((double)d0 * (2 * kPi));
                        float theta = (float)((double)d1 * kPi);
                        lp = V3(-slrSin(phi) * slrSin(theta), slrCos(theta), slrCos(phi) * slrSin(theta));
                        lgn = -lp;
                        lf.x = normalize(V3(-slrCos(phi), 0.0f, -slrSin(phi)));
                        lf.z = lgn;
                        lf.y = cross(lf.z, lf.x);
                        areaPDF = (float)((double)uvPDF / (2 * kPi * kPi * (double)slrSin(theta)));
                        M = envEmittanceS<S>(sc, (float)((double)phi / (2 * kPi)), (float)((double)theta / kPi), wlOffset);
                        sdir = normalize(lp);                              // Scene::testVisibility :421-423: [eps, FLT_MAX]
                        shadowTmax = 3.402823466e+38f;
                    }
                    else {
                        uint32_t li = selectLight(sc, lightCDF, lightPMF, uSel, &lightProb);
                        lightProb *= 1.0f;
                        if (sc.hasEnv) lightProb *= sc.aggImportance / (sc.aggImportance + 1.0f);
                        // Triangle::sample TriangleMesh.cpp:224-255
                        const float4* lt = (LDS_TABLES ? lds.lights : reinterpret_cast<const float4*>(sc.lightTris)) + (size_t)li * 9;
                        float4 l0 = lt[0], l1 = lt[1], l2 = lt[2], l3 = lt[3], l4 = lt[4], l5 = lt[5], l6 = lt[6], l7 = lt[7], l8 = lt[8];
                        float su1 = sqrtf(lu0);
                        float b0 = 1.0f - su1;
                        float b1 = lu1 * su1;
                        float b2 = 1.0f - b0 - b1;
                        lp = b0 * xyz(l0) + b1 * xyz(l1) + b2 * xyz(l2);
                        lgn = V3(l3.w, l4.w, l5.w);
                        lf.z = normalize(b0 * xyz(l3) + b1 * xyz(l4) + b2 * xyz(l5));
                        lf.x = normalize(b0 * xyz(l6) + b1 * xyz(l7) + b2 * xyz(l8));
                        lf.y = cross(lf.z, lf.x);
                        areaPDF = l2.w;
                        const uint32_t lmat = __float_as_uint(l1.w);
                        M = MatIO<S>::template emittance<LDS_TABLES>(sc, lds.mats, lmat, wlOffset);
                        // shadow ray of Scene::testVisibility SurfaceObject.cpp:425-426
                        float dist = length(surf.p - lp);
                        sdir = (lp - surf.p) / dist;
                        shadowTmax = dist * (1 - kRayEpsilon);
                    }
                    // (written for a sample that turns out dead as well, below: nothing reads it then.  Holding the direction back until that
                    // is known costs k_shade's tight instantiations the register that decides their fourth wave: measured)
                    pb.shadowDir[slot] = make_float4(sdir.x, sdir.y, sdir.z, shadowTmax);
                    if constexpr (!kSkipDead) emitShadow = true;
                    // contribution if visible :181-202
                    float dist2;
                    V3 shadowDir;
                    if (pickEnv) { dist2 = 1.0f; shadowDir = normalize(lp); }   // SurfacePoint::getDirectionFrom geometry.cpp:32-37
                    else {
                        V3 dvec = lp - surf.p;
                        dist2 = sqLength(dvec);
                        shadowDir = dvec / sqrtf(dist2);
                    }
                    V3 shadowDir_l = lf.toLocal(-shadowDir);
                    V3 shadowDir_sn = surf.frame.toLocal(shadowDir);
                    S Le = M * S(pickEnv ? (float)(1.0 / kPi) : diffuseEDF(shadowDir_l));
                    float lightPDF = lightProb * areaPDF;
                    float pdfDir = 0.0f;
                    S fs;
                    bool evaluated = false;
                    if constexpr (MULTI) {
                        if (isMulti) {
                            const MultiBSDF<S, decltype(loadComponent)> multi = {multiTree, wlSel, loadComponent};
                            fs = multi.evaluate(type, dirOut_sn, gNorm_sn, shadowDir_sn, wl, &pdfDir);
                            evaluated = true;
                        }
                    }
                    if (!evaluated) fs = bsdfEvaluate<S, MF>(m, type, dirOut_sn, gNorm_sn, shadowDir_sn, wl, &pdfDir);
                    float cosLight = absDot(-shadowDir, lgn);
                    float bsdfPDF = pdfDir * cosLight / dist2;
                    float MISWeight = 1.0f;
                    if (!isinf(areaPDF))
                        MISWeight = (lightPDF * lightPDF) / (lightPDF * lightPDF + bsdfPDF * bsdfPDF);
                    float G = absDot(shadowDir_sn, gNorm_sn) * cosLight / dist2;
                    S contrib = alpha * Le * fs * (G * MISWeight / lightPDF);
                    if constexpr (kSkipDead) {
                        // The reference traces every shadow ray and then adds what came back.  Where the sample is a zero that leaves the
                        // Kahan pair as it is (deadLightSample; this step is the last of the visit to touch the pair, the resolve of the next
                        // visit the first), nothing can depend on the ray: no pending sample, no queue entry, no flag bit —
                        // and a path whose BSDF sample fails below ends here instead of waiting an iteration for it.  The ray still counts
                        // as cast (T_SHADOW_RAYS, by the caller).  RenderParams::traceAllShadows keeps every ray: the comparator.
                        const bool dead = !rp.traceAllShadows && deadLightSample(sp.r, sp.c, contrib);
                        if (dead) *deadShadow = true;
                        else {
                            SpecIO<S>::store(pb.nee, nullptr, slot, rp.numSlots, contrib, 0.0f);
                            emitShadow = true;
                        }
                    }
                    else SpecIO<S>::store(pb.nee, nullptr, slot, rp.numSlots, contrib, 0.0f);
                }
                float uComp = rng.nextFloat();
                float u0 = rng.nextFloat();
                float u1 = rng.nextFloat();
                BsdfSample bs;
                S fs;
                bool sampled = false;
                if constexpr (MULTI) {
                    if (isMulti) {
                        const MultiBSDF<S, decltype(loadComponent)> multi = {multiTree, wlSel, loadComponent};
                        fs = multi.sample(type, dirOut_sn, gNorm_sn, wl, uComp, u0, u1, &bs);
                        sampled = true;
                    }
                }
                if (!sampled) fs = bsdfSample<S, MF>(m, type, dirOut_sn, gNorm_sn, wl, uComp, u0, u1, &bs);
                if (fs.isZero() || bs.dirPDF == 0.0f) {
                    finish = true;                                         // :209
                }
                else {
                    if (bs.dirType & DT_Dispersive) {                      // :211-214
                        bs.dirPDF /= S::N;                                 // WavelengthSamples::NumComponents
                        wlSel = 1;
                    }
                    alpha = alpha * (fs * absDot(bs.dir_sn, gNorm_sn) / bs.dirPDF);     // :215
                    rayDir = surf.frame.fromLocal(bs.dir_sn);
                    rayOrg = surf.p;                                       // :221 Ray(p, dirIn, time, eps)
                    rayTmin = kRayEpsilon;
                    bsdfPDFprev = bs.dirPDF;
                    flags = F_MAKE((uint32_t)ST_NEXT_HIT, pathLength, wl, wlSel, dtIsDelta(bs.dirType) ? 1u : 0u, emitShadow ? 1u : 0u);
                    emitExt = true;
                }
                // the shadow ray starts at the shading point, which is also the next ray's origin
                if (emitShadow && !emitExt) pb.rayOrg[(size_t)slot * pb.rayStride] = make_float4(surf.p.x, surf.p.y, surf.p.z, kRayEpsilon);
            }
        }

        // ---- 4. path finished ----------------------------------------------------------------------------
        if (finish && emitShadow) {
            // the NEE of this bounce is still in flight: finish next iteration
            flags = F_MAKE((uint32_t)ST_FINISH, pathLength, wl, wlSel, 0u, 1u);
        }
        else if (finish) {
            flags = F_MAKE((uint32_t)ST_REGEN, 0u, 0u, 0u, 0u, 0u) | (1u << 15);
            emitRegen = true;
        }

        // ---- store path state ---------------------------------------------------------------------------
        // TIGHT: the records' addresses are made again, from a copy of the slot index that the compiler cannot trace back to the index the
        // state loads used; otherwise it keeps the loads' seven per-lane 64-bit addresses in registers through the whole visit
        uint32_t slotOut = slot;
        if constexpr (TIGHT) asm volatile("" : "+v"(slotOut));
        flags |= sp.validBits();
        if (FUSED && emitRegen) {
            radiance = sp.total();                 // accumulated by the caller: nothing of this path needs to reach HBM any more
        }
        else {
            pb.flags[slotOut] = flags;
            sp.end(pb, slotOut, rp.numSlots, !emitRegen);
        }
        if (!emitRegen) {
            pb.rng[(size_t)slotOut * pb.hdrStride] = make_uint4(rng.s0, rng.s1, rng.s2, rng.s3);
            SpecIO<S>::store(pb.alpha, pb.pdfPrev, slotOut, rp.numSlots, alpha, bsdfPDFprev);
        }
        if (emitExt) {
            pb.rayOrg[(size_t)slotOut * pb.rayStride] = make_float4(rayOrg.x, rayOrg.y, rayOrg.z, rayTmin);
            pb.rayDir[(size_t)slotOut * pb.rayStride] = make_float4(rayDir.x, rayDir.y, rayDir.z, INFINITY);
        }
    }
}

} // namespace slrhip
