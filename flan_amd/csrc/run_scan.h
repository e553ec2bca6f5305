// run_scan.h -- what the scans over frames (compress.hip, filter.hip) share around their own arithmetic, written ONCE.  DESIGN.md section 4.14.
//
// A first-order recurrence over the frames of a row is a scan of maps of its state.  A lane owns a RUN of consecutive frames and reduces
// it to one fp64 map (the file's summarise); block_scan composes the maps over the wavefront (__shfl_up) and the block (LDS) and leaves
// the block's total; k_scan_carry (one block per row) turns the totals into the state at every block's first frame; the file's replay
// kernel scans the block again and replays every run in fp32 from the state carried in.  Every composition runs in a fixed order.
// A file brings: a map type M with then( earlier, later ), shfl_up( M, off ), set_identity( M & ) and apply( M, state ), found here by
// argument-dependent lookup; a summarise; a replay.
#pragma once
#include "flanhip_internal.h"

namespace flanhip {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_RUN = 16;              // frames per lane: 4096 per block, 703 blocks per row for a minute at 48 kHz
constexpr int SCAN_MAX_RUN = 64;

// the run used for a forced one (a file's debug hook; 0: the library's choice)
inline int scan_run( int forced ) { return forced > 0 ? std::min( forced, SCAN_MAX_RUN ) : SCAN_RUN; }
// blocks per row of n frames
inline int64_t scan_blocks( int64_t n, int run )
	{
	const int64_t per_block = int64_t( SCAN_THREADS ) * run;
	return ( n + per_block - 1 ) / per_block;
	}

// Scan of one map per thread over the block, in thread order: excl = the maps of all earlier threads composed, total = the block's.
// Every thread of the block calls it.
template<typename M>
__device__ __forceinline__ void block_scan( const M & mine, M * s_tot, M & excl, M & total )
	{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	M inc = mine;
	#pragma unroll
	for( int off = 1; off < 64; off <<= 1 )
		{
		const M o = shfl_up( inc, off );
		if( lane >= off ) inc = then( o, inc );
		}
	if( lane == 63 ) s_tot[wave] = inc;
	__syncthreads();
	M prev = shfl_up( inc, 1 );
	if( lane == 0 ) set_identity( prev );
	M pre; set_identity( pre );
	for( int w = 0; w < wave; ++w ) pre = then( pre, s_tot[w] );
	excl = then( pre, prev );
	total = s_tot[0];
	#pragma unroll
	for( int w = 1; w < SCAN_WAVES; ++w ) total = then( total, s_tot[w] );
	__syncthreads();
	}

// the first `valid` of four consecutive floats from frame f of a row (VEC: all four: f a multiple of 4, the row 16-byte aligned and a run
// whole quads, or the row padded to one); otherwise nothing past the run is read: those frames are the next lane's, which may be writing
// them when dst is src
template<bool VEC>
__device__ __forceinline__ void load4( const float * p, int64_t f, int valid, float ( &v )[4] )
	{
	if constexpr( VEC )
		{
		const float4 q = *reinterpret_cast<const float4*>( p + f );
		v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
		}
	else
		{
		#pragma unroll
		for( int k = 0; k < 4; ++k ) v[k] = k < valid ? p[f + k] : 0.0f;
		}
	}
// the first `valid` of four values to frame f on.  VEC: all four (a run is whole quads then, so valid < 4 only where the quad ends in a
// padded row's padding); otherwise nothing past the run: those frames are the next lane's
template<bool VEC>
__device__ __forceinline__ void store4( float * p, int64_t f, int valid, const float ( &v )[4] )
	{
	if constexpr( VEC ) *reinterpret_cast<float4*>( p + f ) = make_float4( v[0], v[1], v[2], v[3] );
	else
		{
		#pragma unroll
		for( int k = 0; k < 4; ++k ) if( k < valid ) p[f + k] = v[k];
		}
	}

// the run of the calling thread in block `block` of a row of n frames: frames [f0, f0 + len)
__device__ __forceinline__ void lane_run_of( int64_t block, int64_t n, int run, int64_t & f0, int & len )
	{
	f0 = ( block * SCAN_THREADS + threadIdx.x ) * run;
	len = int( std::min<int64_t>( std::max<int64_t>( n - f0, 0 ), run ) );
	}
// one row: the grid is its blocks
__device__ __forceinline__ void lane_run( int64_t n, int run, int64_t & f0, int & len ) { lane_run_of( int64_t( blockIdx.x ), n, run, f0, len ); }
// rows of `blocks` blocks each, the grid flattened: the block's row (its channel) as well
__device__ __forceinline__ void lane_run( int64_t n, int run, int64_t blocks, int64_t & channel, int64_t & f0, int & len )
	{
	channel = int64_t( blockIdx.x ) / blocks;
	lane_run_of( int64_t( blockIdx.x ) - channel * blocks, n, run, f0, len );
	}

// One block per row: the state at the first frame of every block of the row's scan, from the block totals and the state S{} (zero) before
// frame 0.  tot and carry: [rows][blocks]
template<typename M, typename S>
__global__ __launch_bounds__( SCAN_THREADS ) void k_scan_carry( const M * __restrict__ tot, int64_t blocks, S * __restrict__ carry )
	{
	__shared__ M s_tot[SCAN_WAVES];
	tot += int64_t( blockIdx.x ) * blocks;
	carry += int64_t( blockIdx.x ) * blocks;
	S state{};
	for( int64_t base = 0; base < blocks; base += SCAN_THREADS )
		{
		const int64_t b = base + threadIdx.x;
		M mine; set_identity( mine );
		if( b < blocks ) mine = tot[b];
		M excl, total;
		block_scan( mine, s_tot, excl, total );
		if( b < blocks ) carry[b] = apply( excl, state );
		state = apply( total, state );
		}
	}

} // namespace flanhip
