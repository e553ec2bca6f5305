// wavetable.hip -- flan::Wavetable (Wavetable.cpp): a table of single-cycle waveforms cut from an Audio, each Fourier-resampled to one
// wavelength, and its synthesis through WDL_Resampler's 64-tap windowed sinc (WDL/resample.cpp).  DESIGN.md section 4.23.
//   k_wt_resample   resample_waveforms (:67-132): one workgroup per ( channel, waveform slot ).  The n source frames in LDS, the
//                   min( n/2, W/2 ) + 1 bins of the size-n real transform as direct sums (n is any positive integer; fp32 products chained
//                   32 at a time, the chunks added in fp64), the merged real inverse of W points over fft_device.h, the zero-crossing
//                   search by one wavefront, the rotated and scaled store
//   k_wt_synth      synthesize (:266-334): one workgroup per ( run of output frames sharing a coefficient table, channel group ).  The
//                   resampler's input is no buffer: stream sample s >= 31 is sample t = s - 31 of a periodic read of the table, blended
//                   between two neighbouring waveforms with the weights of the block that appended it.  With a row stride of 0 and a phase
//                   offset per channel it is also the loop of Audio::synthesize_spectrum (flanhip_spectrum_synth; spectrum.hip makes its table)
//   k_wt_edit       normalize / remove_dc / add_fades / remove_jumps (:364-451): one workgroup per ( channel, slot )
// The waveform starts (:19-65, :134-218), the table index (:463-488) and the resampler's state (the plan) are host arithmetic.
// Every sum runs in a fixed order and nothing is atomic, so two runs agree bit for bit.
#include "wdl_sinc.h"
#include "fft_device.h"

#include <cstring>

namespace flanhip {

namespace {

constexpr int WT_TAPS = 64;                    // SetMode( true, 1, true ): sinc, the default m_sincsize
using Wt = WdlSinc<WT_TAPS>;
constexpr int WT_THREADS = WDL_THREADS;
constexpr int WT_MIN_W = 64, WT_MAX_W = 8192;  // fft_forward serves 2^4 ... 2^12 complex points; below 64 the search distance is under 6 frames
constexpr int WT_MAX_N = 16384;                // source frames of one waveform: 64 KiB of LDS beside the spectrum at W = 8192
constexpr int WT_TW_LDS_N = 4096;              // up to here the n twiddles sit in LDS behind the samples; a longer table is kept in the workspace
constexpr int WT_CHUNK = 32;                   // fp32 terms chained before they are added in fp64 (as pitch.hip's compute_d)
constexpr int WT_WINDOW_FLOATS = 6144;         // the staged stream window of a run (24 KiB)
constexpr int WT_RUN_OUTPUTS = 2048;           // output frames per run at most
constexpr int64_t WT_MAX_FRAMES = int64_t( 1 ) << 33;
constexpr int64_t WT_MAX_BLOCKS = int64_t( 1 ) << 22;

// ------------------------------------------------------------------------------------------------------------------------------------
// waveform starts: host arithmetic

// snap_frame_to_sample (:19-60), literally.  data: one channel row of n frames, 0 <= frame_to_snap < n.
int32_t wt_snap( const float * data, int64_t n, int32_t frame_to_snap, float snap_height, int32_t search_distance )
	{
	const int32_t left_frame_limit = std::max( frame_to_snap - search_distance, 0 );
	const int32_t right_frame_limit = std::min<int64_t>( int64_t( frame_to_snap ) + search_distance, n - 1 );
	const bool is_above = data[frame_to_snap] > snap_height;
	for( int32_t search_offset = 0; search_offset <= search_distance; ++search_offset )
		{
		const int32_t left_search_frame = frame_to_snap - search_offset;
		if( left_search_frame >= left_frame_limit && ( data[left_search_frame] > snap_height ) != is_above )
			return left_search_frame + 1;
		const int64_t right_search_frame = int64_t( frame_to_snap ) + search_offset;
		if( right_search_frame < right_frame_limit && ( data[right_search_frame] > snap_height ) != is_above )
			return int32_t( right_search_frame );
		}
	// the search failed: the frame nearest to the crossing, slightly preferring frames near the initial one.  A distance of 0 makes r
	// NaN at frame_to_snap, every comparison false, and frame_to_snap the answer
	auto norm = [&]( int32_t f )
		{
		const float m = 1.0f;
		const float r = 1.0f + m * float( std::abs( f - frame_to_snap ) ) / float( search_distance );
		return std::abs( data[f] - snap_height ) * r;
		};
	int32_t current_best_frame = frame_to_snap;
	float current_best_sample_distance = norm( frame_to_snap );
	for( int32_t search_frame = left_frame_limit; search_frame <= right_frame_limit; ++search_frame )
		{
		const float current_sample_distance = norm( search_frame );
		if( current_sample_distance < current_best_sample_distance )
			{
			current_best_frame = search_frame;
			current_best_sample_distance = current_sample_distance;
			}
		}
	return current_best_frame;
	}

int32_t wt_trunc( float v )                    // Frame( float ) where the reference's conversion is defined; what no Frame holds saturates
	{
	if( !( v == v ) ) return 0;
	if( v >= 2147483648.0f ) return INT32_MAX;
	if( v <= -2147483648.0f ) return INT32_MIN;
	return int32_t( v );
	}

// ------------------------------------------------------------------------------------------------------------------------------------
// table construction

struct WtWave { int32_t start, n; int64_t tw_off; };       // tw_off: the waveform's twiddle row in the workspace (cf units) where n > WT_TW_LDS_N

struct WtResamplePlan
	{
	std::vector<WtWave> waves;                 // [ch][slots]
	int64_t slots = 0, tw_total = 0;
	int32_t max_n = 0;
	};

size_t wt_resample_lds( int W, int max_n )
	{
	const int C = W / 2;
	const size_t z = sizeof( cf ) * size_t( C + 2 );
	const size_t a = sizeof( float ) * size_t( ( max_n + 3 ) & ~3 ) + sizeof( cf ) * size_t( std::min( max_n, WT_TW_LDS_N ) );
	const size_t b = sizeof( cf ) * size_t( padded_len( C ) + C );
	return z + std::max( a, b );
	}

int wt_resample_check( const void * audio, int64_t ch, int64_t frames, const int32_t * starts, const int64_t * counts, int32_t W, const void * table )
	{
	FLANHIP_REQUIRE( audio && starts && counts && table, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && frames > 0 && W > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( is_pow2( W ) && W >= WT_MIN_W && W <= WT_MAX_W, FLANHIP_ERR_UNSUPPORTED, "the wavelength must be a power of two in 64 ... 8192" );
	FLANHIP_REQUIRE( ch <= ( 1 << 16 ) && frames < ( int64_t( 1 ) << 31 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

int wt_resample_plan( int64_t ch, int64_t frames, const int32_t * starts, const int64_t * counts, WtResamplePlan * p )
	{
	int64_t slots = 0;
	for( int64_t c = 0; c < ch; ++c )
		{
		FLANHIP_REQUIRE( counts[c] > 0, FLANHIP_ERR_INVALID_ARG, "a channel without waveform starts" );
		slots = std::max( slots, counts[c] );
		}
	FLANHIP_REQUIRE( slots * ch < ( int64_t( 1 ) << 28 ), FLANHIP_ERR_UNSUPPORTED, "too many waveforms" );
	p->slots = slots;
	p->waves.assign( size_t( ch * slots ), WtWave{ 0, 0, 0 } );
	const int32_t * s = starts;
	for( int64_t c = 0; c < ch; ++c )
		{
		for( int64_t w = 0; w + 1 < counts[c]; ++w )
			{
			const int64_t a = s[w], n = int64_t( s[w + 1] ) - a;
			if( n <= 0 ) continue;                                                  // the slot stays 0 (the reference would plan a size-0 transform)
			FLANHIP_REQUIRE( a >= 0 && a + n <= frames, FLANHIP_ERR_INVALID_ARG, "a waveform leaves the source" );
			FLANHIP_REQUIRE( n <= WT_MAX_N, FLANHIP_ERR_UNSUPPORTED, "a waveform of more than 16384 source frames" );
			WtWave & v = p->waves[size_t( c * slots + w )];
			v.start = int32_t( a ); v.n = int32_t( n );
			if( n > WT_TW_LDS_N ) { v.tw_off = p->tw_total; p->tw_total += n; }
			p->max_n = std::max( p->max_n, int32_t( n ) );
			}
		s += counts[c];
		}
	return FLANHIP_OK;
	}

struct WtResampleLayout { size_t wave_off, tw_off, total; };
WtResampleLayout wt_resample_layout( const WtResamplePlan & p )
	{
	WtResampleLayout l;
	l.wave_off = 0;
	l.tw_off = ( sizeof( WtWave ) * p.waves.size() + 15 ) & ~size_t( 15 );
	l.total = l.tw_off + sizeof( cf ) * size_t( p.tw_total );
	return l;
	}

// grid: ch x slots.  table float[ch][slots W], rot int32[ch][slots] or null.  Dynamic LDS: Z cf[C + 2], then EITHER the samples
// float[n rounded up to 4] and (n <= WT_TW_LDS_N) their twiddles cf[n] OR the inverse's buffer cf[padded_len( C )] and twiddles cf[C].
template<int LOG2C>
__global__ __launch_bounds__( WT_THREADS ) void k_wt_resample( const float * __restrict__ audio, int64_t frames, const WtWave * __restrict__ waves,
	int64_t slots, float * __restrict__ table, int32_t * __restrict__ rot, const cf * __restrict__ g_tw, const cf * __restrict__ g_tw2,
	cf * __restrict__ g_twid )
	{
	constexpr int C = 1 << LOG2C;
	constexpr int W = 2 * C;
	extern __shared__ __align__( 16 ) char s_raw[];
	__shared__ int s_zc;
	cf * Z = reinterpret_cast<cf*>( s_raw );
	char * U = s_raw + sizeof( cf ) * ( C + 2 );
	const int lane = threadIdx.x;
	const int64_t slot = blockIdx.x;
	const int64_t c = slot / slots;
	const WtWave wave = waves[slot];
	const int n = wave.n;
	float * out = table + slot * W;
	if( n <= 0 )
		{
		for( int f = lane; f < W; f += WT_THREADS ) out[f] = 0.0f;
		if( rot && lane == 0 ) rot[slot] = 0;
		return;
		}

	// the samples, and exp( -2 pi i m / n ) for m < n from fp64
	float * xs = reinterpret_cast<float*>( U );
	cf * tws = n <= WT_TW_LDS_N ? reinterpret_cast<cf*>( U + sizeof( float ) * ( ( n + 3 ) & ~3 ) ) : g_twid + wave.tw_off;
	const float * x = audio + c * frames + wave.start;
	for( int j = lane; j < n; j += WT_THREADS )
		{
		xs[j] = x[j];
		double sn, cs;
		sincospi( 2.0 * double( j ) / double( n ), &sn, &cs );
		tws[j] = mk( float( cs ), float( -sn ) );
		}
	__syncthreads();

	// Z[k] = sum_j x[j] exp( -2 pi i j k / n ) for k <= min( n/2, C ) (the reference copies n/2 + 1 bins even past the end of its buffer;
	// here at most C + 1), zeros above
	const int K = ( n / 2 < C ? n / 2 : C ) + 1;
	for( int k = lane; k <= C; k += WT_THREADS )
		{
		double re = 0.0, im = 0.0;
		if( k < K )
			{
			int idx = 0;                                                          // j k mod n
			for( int j0 = 0; j0 < n; j0 += WT_CHUNK )
				{
				const int j1 = j0 + WT_CHUNK < n ? j0 + WT_CHUNK : n;
				float cr = 0.0f, ci = 0.0f;
				for( int j = j0; j < j1; ++j )
					{
					const float v = xs[j];
					const cf w = tws[idx];
					cr = __builtin_fmaf( v, w.x, cr );
					ci = __builtin_fmaf( v, w.y, ci );
					idx += k;
					if( idx >= n ) idx -= n;
					}
				re += double( cr ); im += double( ci );
				}
			}
		Z[k] = mk( float( re ), float( im ) );
		}
	__syncthreads();                                                             // Z is whole; the samples and their twiddles are read

	// the unnormalised c2r of W points as k_conv_inverse does it: Z = A + iB stored conjugated, one forward FFT of C points
	cf * buf = reinterpret_cast<cf*>( U );
	cf * tw = buf + padded_len( C );
	for( int k = lane; k < C; k += WT_THREADS )
		{
		tw[k] = g_tw[k];
		cf xk = Z[k], xm = Z[C - k];
		if( k == 0 ) { xk.y = 0.0f; xm.y = 0.0f; }                               // c2r ignores the imaginary parts of bins 0 and W/2
		const float ax = xk.x + xm.x, ay = xk.y - xm.y;
		const float dx = xk.x - xm.x, dy = xk.y + xm.y;
		const cf w2q = g_tw2[k];
		const float cc = w2q.x, ss = -w2q.y;
		const float bx = __builtin_fmaf( cc, dx, -( ss * dy ) ), by = __builtin_fmaf( cc, dy, ss * dx );
		buf[PAD( k )] = mk( ax - by, -( ay + bx ) );
		}
	__syncthreads();
	fft_forward<LOG2C, WT_THREADS>( buf, tw, lane );                             // (ends with a barrier)
	auto y = [&]( int t ) { const cf F = buf[PAD( t >> 1 )]; return ( t & 1 ) ? -F.y : F.x; };

	// :105-120: offsets 1 ... search_distance, W - offset before offset; candidate 2 ( offset - 1 ) + side in that order, the first that differs
	if( lane < 64 )
		{
		const int search_distance = int( float( W ) * 0.1f );
		const bool is_above = y( 0 ) > 0.0f;
		int best = INT32_MAX;
		for( int q = lane; q < 2 * search_distance && best == INT32_MAX; q += 64 )
			{
			const int offset = ( q >> 1 ) + 1;
			const int t = ( q & 1 ) ? offset : W - offset;
			if( ( y( t ) > 0.0f ) != is_above ) best = q;
			}
		#pragma unroll
		for( int off = 32; off > 0; off >>= 1 ) { const int o = __shfl_xor( best, off ); best = o < best ? o : best; }
		if( lane == 0 )
			{
			int zc = 0;
			if( best != INT32_MAX ) { const int offset = ( best >> 1 ) + 1; zc = ( best & 1 ) ? offset : W - offset; }
			s_zc = zc;
			if( rot ) rot[slot] = zc;
			}
		}
	__syncthreads();
	const int zc = s_zc;
	const float scale = sqrtf( float( n * n ) );                                 // :125
	for( int f = lane; f < W; f += WT_THREADS ) out[f] = y( ( zc + f ) & ( W - 1 ) ) / scale;
	}

int launch_wt_resample( const float * d_audio, int64_t ch, int64_t frames, int32_t W, const WtResamplePlan & p, float * d_table, int32_t * d_rot,
	void * d_ws, hipStream_t s )
	{
	const WtResampleLayout l = wt_resample_layout( p );
	FLANHIP_CHECK( hipMemcpyAsync( ws_at<char>( d_ws, l.wave_off ), p.waves.data(), sizeof( WtWave ) * p.waves.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );                                  // the host vector may go once the copy has read it
	std::shared_ptr<const PlanRef> plan;
	if( int rc = get_plan( W, W, &plan ) ) return rc;                            // tw [W/2] and tw2 [W/2 + 1] of a W-point real transform
	const size_t lds = wt_resample_lds( W, p.max_n );
	const int64_t grid = ch * p.slots;
	const WtWave * d_waves = ws_at<WtWave>( d_ws, l.wave_off );
	cf * d_twid = ws_at<cf>( d_ws, l.tw_off );
	#define WT_CASE( L ) case L: return launch_kernel( "wavetable_resample", k_wt_resample<L>, grid, WT_THREADS, lds, s, d_audio, frames, d_waves, p.slots, d_table, d_rot, (const cf*) plan->plan.d_tw, (const cf*) plan->plan.d_tw2, d_twid );
	switch( ilog2( W ) - 1 )
		{
		WT_CASE( 5 ) WT_CASE( 6 ) WT_CASE( 7 ) WT_CASE( 8 ) WT_CASE( 9 ) WT_CASE( 10 ) WT_CASE( 11 ) WT_CASE( 12 )
		default: set_error( "wavetable_resample: unsupported wavelength %d", int( W ) ); return FLANHIP_ERR_UNSUPPORTED;
		}
	#undef WT_CASE
	}

// ------------------------------------------------------------------------------------------------------------------------------------
// synthesis

struct WtBlock                                 // one pass of the loop of :295-330: SetRates, ResamplePrepare, the copy, ResampleOut
	{
	int64_t offset;                            // stream index of the buffer's first sample
	double fracpos;                            // srcpos of the block's first output sample, relative to offset
	double ratio;
	double filtpos;
	int64_t first_out;
	int64_t in_start;                          // input samples appended before this block; its phase_frame (:329) is in_start % W
	double last_pos;                           // srcpos of the block's last output sample (fracpos after num_out - 1 additions of ratio)
	int32_t oversize, ideal;
	int32_t wanted, num_out;
	};

struct WtRun                                   // consecutive output frames that share ( filtpos, oversize, ideal ) and whose taps fit the staged window
	{
	int64_t first_out;
	int64_t j0;                                // first_out is output j0 of block first_block (0 unless the block was cut into pieces) ...
	double start_pos;                          // ... whose srcpos is this: the block's chain of additions up to j0
	int64_t first_block;                       // the block of first_out; the run's frames lie in blocks first_block ... first_block + num_blocks - 1
	int64_t win_start;                         // stream index of the first staged sample
	int64_t q_first;                           // the blocks that appended the window's samples: q_first ... q_first + q_count - 1
	double filtpos;
	int32_t num_out, num_blocks;
	int32_t win_len, q_count;
	int32_t oversize, ideal;
	};
static_assert( sizeof( WtBlock ) == 72 && sizeof( WtRun ) == 80, "the device reads these records as the host lays them out" );

struct WtPlan { std::vector<WtBlock> blocks; int64_t total_in = 0; };

int wt_synth_check( int64_t out_frames, float sr, int32_t W, int64_t g, const float * freq, int64_t freq_count )
	{
	FLANHIP_REQUIRE( freq, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( out_frames > 0 && W > 0 && freq_count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( g >= 1, FLANHIP_ERR_INVALID_ARG, "a granularity below one frame (the reference's loop would not end)" );
	FLANHIP_REQUIRE( out_frames <= WT_MAX_FRAMES && g <= WT_MAX_FRAMES && W <= ( 1 << 24 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// The loop of :293-330 with the state of ResamplePrepare (:1218-1265) and ResampleOut (:1313-1343, :1558-1566) in fp64, the reference's own
// chain of srcpos += ratio.  ResampleOut is asked for all the frames that remain, so a block ends where its input does
// (ipos >= filtlen - 1, :1343), not after g frames: block b + 1 begins where block b stopped.
// rate_out: SetRates' second argument (:307), from the caller: max( sr / W, 1 ) for a wavetable (:299), max( fundamental, 1 ) for
// Audio::synthesize_spectrum (AudioSynthesis.cpp:247)
int wt_synth_plan( int64_t out_frames, double rate_out, int64_t g, const float * freq, int64_t freq_count, WtPlan * plan )
	{
	double fracpos = 0.0;
	int64_t S = 0, offset = 0, out = 0, in_total = 0;
	bool first = true;
	int idle = 0;
	while( out < out_frames )
		{
		const float f = freq[std::min( out, freq_count - 1 )];
		FLANHIP_REQUIRE( std::isfinite( f ), FLANHIP_ERR_INVALID_ARG, "a frequency that is not finite" );
		const double rate_in = std::max( double( f ), 1.0 );                     // :300, SetRates' first argument
		const double ratio = rate_in / rate_out;
		if( S < Wt::PRELUDE )                                                    // :1226-1237
			{
			// later than the first call the reference declares samples its buffer no longer holds (what an earlier block left there)
			FLANHIP_REQUIRE( first, FLANHIP_ERR_UNSUPPORTED, "a rate ratio above 34 after the first block: the reference's resampler then reads stale samples" );
			S = Wt::PRELUDE;
			}
		first = false;
		const double span = ratio * double( g );
		FLANHIP_REQUIRE( span < 1.0e9, FLANHIP_ERR_UNSUPPORTED, "ratio times granularity out of range" );
		const int64_t wanted = std::max<int64_t>( int64_t( span ) + 4 + WT_TAPS - S, 0 );      // :1241-1244
		S += wanted;                                                             // :1295
		WtBlock b{};
		b.offset = offset; b.fracpos = fracpos; b.ratio = ratio; b.first_out = out; b.in_start = in_total; b.wanted = int32_t( wanted );
		wdl_table_shape( rate_in, rate_out, ratio, &b.filtpos, &b.oversize, &b.ideal );
		const int64_t limit = S - WT_TAPS - 1;                                   // filtlen - 1
		const int64_t remaining = out_frames - out;
		double srcpos = fracpos;
		int64_t count = 0;
		while( count < remaining && int64_t( srcpos ) < limit ) { b.last_pos = srcpos; srcpos += ratio; ++count; }
		b.num_out = int32_t( count );
		FLANHIP_REQUIRE( count < ( int64_t( 1 ) << 31 ), FLANHIP_ERR_UNSUPPORTED, "a block of more than 2^31 frames" );
		plan->blocks.push_back( b );
		const int64_t isrcpos = wdl_hand_over( srcpos, S, b.ideal, b.oversize, &fracpos );
		S -= isrcpos;
		offset += isrcpos;
		in_total += wanted;
		out += count;
		idle = count ? 0 : idle + 1;
		FLANHIP_REQUIRE( idle < 4, FLANHIP_ERR_UNSUPPORTED, "the resampler delivers nothing" );
		FLANHIP_REQUIRE( int64_t( plan->blocks.size() ) <= WT_MAX_BLOCKS, FLANHIP_ERR_UNSUPPORTED, "more than 2^22 blocks (granularity too fine for this length)" );
		}
	plan->total_in = in_total;
	return FLANHIP_OK;                                                           // out == out_frames: every output frame belongs to a block
	}

inline double wt_rate_out( float sr, int32_t W ) { return std::max( double( sr ) / double( W ), 1.0 ); }     // :299

// the block that appended input sample t: the last q with in_start[q] <= t
int64_t wt_owner( const std::vector<WtBlock> & blocks, int64_t t )
	{
	int64_t lo = 0, hi = int64_t( blocks.size() ) - 1;
	while( lo < hi )
		{
		const int64_t mid = ( lo + hi + 1 ) / 2;
		if( blocks[size_t( mid )].in_start <= t ) lo = mid; else hi = mid - 1;
		}
	return lo;
	}

void wt_runs( const WtPlan & plan, std::vector<WtRun> * runs )
	{
	const std::vector<WtBlock> & bl = plan.blocks;
	// stream index one past the taps of an output at srcpos `pos` of block b (+ 2: the window never ends on the last tap)
	auto taps_end = [&]( const WtBlock & b, double pos ) { return b.offset + int64_t( pos ) + WT_TAPS + 2; };
	auto close = [&]( WtRun r, int64_t end )
		{
		r.win_len = int32_t( end - r.win_start );
		const int64_t t0 = std::max<int64_t>( r.win_start - Wt::PRELUDE, 0 ), t1 = std::max<int64_t>( end - 1 - Wt::PRELUDE, 0 );
		r.q_first = wt_owner( bl, t0 );
		r.q_count = int32_t( wt_owner( bl, t1 ) - r.q_first + 1 );
		runs->push_back( r );
		};
	size_t i = 0;
	while( i < bl.size() )
		{
		const WtBlock & a = bl[i];
		if( a.num_out == 0 ) { ++i; continue; }
		WtRun r{};
		r.first_out = a.first_out; r.first_block = int64_t( i ); r.oversize = a.oversize; r.ideal = a.ideal; r.filtpos = a.filtpos;
		r.j0 = 0; r.start_pos = a.fracpos;
		r.win_start = a.offset + int64_t( a.fracpos );
		if( a.num_out > WT_RUN_OUTPUTS || taps_end( a, a.last_pos ) - r.win_start > WT_WINDOW_FLOATS )
			{
			// one block alone is too much: cut it into pieces along its own chain of positions (a piece of one frame always fits: 64 + 2 taps)
			double pos = a.fracpos, last = a.fracpos;
			WtRun p = r;
			p.num_blocks = 1;
			int64_t outs = 0;
			for( int64_t j = 0; j < a.num_out; ++j )
				{
				if( outs && ( outs == WT_RUN_OUTPUTS || taps_end( a, pos ) - p.win_start > WT_WINDOW_FLOATS ) )
					{
					p.num_out = int32_t( outs );
					close( p, taps_end( a, last ) );
					p.first_out = a.first_out + j; p.j0 = j; p.start_pos = pos; p.win_start = a.offset + int64_t( pos );
					outs = 0;
					}
				last = pos; pos += a.ratio; ++outs;
				}
			p.num_out = int32_t( outs );
			close( p, taps_end( a, last ) );
			++i;
			continue;
			}
		int64_t end = taps_end( a, a.last_pos ), outs = a.num_out;
		size_t k = i + 1;
		while( k < bl.size() )
			{
			const WtBlock & b = bl[k];
			if( b.num_out == 0 ) { ++k; continue; }
			if( !wdl_same_table( a, b ) ) break;
			const int64_t e = std::max( end, taps_end( b, b.last_pos ) );
			if( outs + b.num_out > WT_RUN_OUTPUTS || e - r.win_start > WT_WINDOW_FLOATS ) break;
			end = e; outs += b.num_out; ++k;
			}
		r.num_out = int32_t( outs ); r.num_blocks = int32_t( k - i );
		close( r, end );
		i = k;
		}
	}

struct WtSynthLayout { WdlLayout wdl; size_t index_off, total; };
WtSynthLayout wt_synth_layout( int64_t ch, int64_t num_blocks, int64_t num_runs )
	{
	WtSynthLayout l;
	l.wdl = wdl_layout<WT_TAPS>( sizeof( WtBlock ), num_blocks, sizeof( WtRun ), num_runs );
	l.index_off = ( l.wdl.total + 15 ) & ~size_t( 15 );
	l.total = l.index_off + sizeof( float ) * size_t( ch ) * size_t( num_blocks );
	return l;
	}

// stream sample s of channel row `tab` (float[slots W]): 31 zeros, then input sample t = s - 31 (read at phase ( t + jump ) % W), appended by the last block q of
// [q_lo, q_hi] with in_start[q] <= t: the blend of :316-318 (SMOOTH) or the left waveform alone (:322-323), every operation rounded
template<bool SMOOTH>
__device__ __forceinline__ float wt_stream( const float * __restrict__ tab, int W, const WtBlock * __restrict__ blocks, const float * __restrict__ index,
	int64_t q_lo, int64_t q_hi, int64_t total_in, int64_t s, int64_t jump )
	{
	const int64_t t = s - Wt::PRELUDE;
	if( t < 0 || t >= total_in ) return 0.0f;
	int64_t lo = q_lo, hi = q_hi;
	while( lo < hi )
		{
		const int64_t mid = ( lo + hi + 1 ) >> 1;
		if( blocks[mid].in_start <= t ) lo = mid; else hi = mid - 1;
		}
	const float idx = index[lo];
	const float fl = floorf( idx );
	const int phase = int( ( t + jump ) % W );
	const float left = tab[phase + W * int( fl )];
	if( !SMOOTH ) return left;
	const float rem = __fsub_rn( idx, fl );
	const float right = tab[phase + W * int( ceilf( idx ) )];
	return __fadd_rn( __fmul_rn( __fsub_rn( 1.0f, rem ), left ), __fmul_rn( rem, right ) );
	}

// grid: runs x channel groups of `cpw` channels.  table: channel c's row of slots W floats starts at c row_stride (slots W; 0: every channel reads
// row 0), jump int32[ch] or null: the channel's phase offset, index float[ch][num_blocks], out float[ch][out_frames].
template<bool SMOOTH>
__global__ __launch_bounds__( WT_THREADS ) void k_wt_synth( const float * __restrict__ table, int64_t ch, int64_t row_stride, const int32_t * __restrict__ jump, int W, int64_t out_frames,
	const WtBlock * __restrict__ blocks, int64_t num_blocks, int64_t total_in, const WtRun * __restrict__ runs, const float * __restrict__ index,
	const double * __restrict__ win, int64_t groups, int cpw, float * __restrict__ out )
	{
	__shared__ float s_tab[Wt::TABLE_FLOATS];
	__shared__ float s_in[WT_WINDOW_FLOATS];
	__shared__ double s_red[WT_THREADS];
	__shared__ double s_pos[WT_RUN_OUTPUTS];
	const int lane = threadIdx.x;
	const int64_t run_index = int64_t( blockIdx.x ) / groups;
	const int64_t c0 = ( int64_t( blockIdx.x ) - run_index * groups ) * cpw;
	const WtRun run = runs[run_index];
	const int oversize = run.oversize;
	// srcpos of every output of the run, by the reference's own chain of srcpos += ratio (:1313-1343): one lane per block walks it
	for( int bi = lane; bi < run.num_blocks; bi += WT_THREADS )
		{
		const WtBlock b = blocks[run.first_block + bi];
		const int64_t j = bi == 0 ? run.j0 : 0;
		double p = bi == 0 ? run.start_pos : b.fracpos;
		int64_t at = b.first_out + j - run.first_out;
		const int64_t stop = b.first_out + b.num_out - run.first_out;
		const int64_t end = stop < run.num_out ? stop : run.num_out;
		for( ; at < end; ++at ) { s_pos[at] = p; p += b.ratio; }
		}
	wdl_build_table<WT_TAPS>( s_tab, s_red, win + size_t( oversize - 1 ) * Wt::WIN_SLOT, oversize, run.filtpos );       // (its barriers publish s_pos)

	const int64_t c1 = c0 + cpw < ch ? c0 + cpw : ch;
	for( int64_t c = c0; c < c1; ++c )
		{
		const float * tab = table + c * row_stride;
		const int64_t jmp = jump ? jump[c] : 0;
		const float * idx = index + c * num_blocks;
		__syncthreads();                                                         // the table is whole; the last channel's reads of s_in are done
		for( int i = lane; i < run.win_len; i += WT_THREADS )
			s_in[i] = wt_stream<SMOOTH>( tab, W, blocks, idx, run.q_first, run.q_first + run.q_count - 1, total_in, run.win_start + i, jmp );
		__syncthreads();
		for( int t = lane; t < run.num_out; t += WT_THREADS )
			{
			const int64_t frame = run.first_out + t;
			int64_t lo = run.first_block, hi = run.first_block + run.num_blocks - 1;          // the last block with first_out <= frame
			while( lo < hi )
				{
				const int64_t mid = ( lo + hi + 1 ) >> 1;
				if( blocks[mid].first_out <= frame ) lo = mid; else hi = mid - 1;
				}
			const WtBlock b = blocks[lo];
			const double srcpos = s_pos[t];
			// every tap lies in the staged window (the run was cut so); the row form of wdl_sample is given an empty row
			out[c * out_frames + frame] = wdl_sample<WT_TAPS>( s_tab, s_in, run.win_start, run.win_len, nullptr, 0, b.offset, srcpos, oversize, run.ideal );
			}
		}
	}

int wt_synth_args( const void * table, int64_t ch, int64_t slots, int32_t W, const float * index, int64_t num_blocks, const WtPlan & plan, const void * out )
	{
	FLANHIP_REQUIRE( table && index && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && slots > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( ch <= ( 1 << 16 ) && slots * int64_t( W ) < ( int64_t( 1 ) << 31 ), FLANHIP_ERR_UNSUPPORTED, "table out of range" );
	FLANHIP_REQUIRE( num_blocks == int64_t( plan.blocks.size() ), FLANHIP_ERR_INVALID_ARG, "one table index per channel and block of the plan is needed" );
	for( int64_t i = 0; i < ch * num_blocks; ++i )
		FLANHIP_REQUIRE( index[i] >= 0.0f && index[i] <= float( slots - 1 ), FLANHIP_ERR_INVALID_ARG, "a table index outside the table" );
	return FLANHIP_OK;
	}

int launch_wt_synth( const float * d_table, int64_t ch, int64_t row_stride, const int32_t * d_jump, int32_t W, int64_t out_frames, const WtPlan & plan,
	const std::vector<WtRun> & runs, const float * index, int smooth, float * d_out, void * d_ws, hipStream_t s )
	{
	const int64_t num_blocks = int64_t( plan.blocks.size() );
	const WtSynthLayout l = wt_synth_layout( ch, num_blocks, int64_t( runs.size() ) );
	char * ws = static_cast<char*>( d_ws );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.wdl.block_off, plan.blocks.data(), sizeof( WtBlock ) * plan.blocks.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.wdl.run_off, runs.data(), sizeof( WtRun ) * runs.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipMemcpyAsync( ws + l.index_off, index, sizeof( float ) * size_t( ch * num_blocks ), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );                                  // the host arrays may go once the copies have read them
	const double * d_win = nullptr;
	if( int rc = wdl_window<WT_TAPS>( "wavetable_synth", d_ws, l.wdl, runs, s, &d_win ) ) return rc;
	int64_t groups = 0;
	const int cpw = wdl_channel_groups( out_frames, runs.size(), ch, &groups );
	const WtBlock * d_blocks = (const WtBlock*) ( ws + l.wdl.block_off );
	const WtRun * d_runs = (const WtRun*) ( ws + l.wdl.run_off );
	const float * d_index = (const float*) ( ws + l.index_off );
	if( smooth )
		return launch_kernel( "wavetable_synth", k_wt_synth<true>, int64_t( runs.size() ) * groups, WT_THREADS, 0, s, d_table, ch, row_stride, d_jump, int( W ), out_frames,
			d_blocks, num_blocks, plan.total_in, d_runs, d_index, d_win, groups, cpw, d_out );
	return launch_kernel( "wavetable_synth", k_wt_synth<false>, int64_t( runs.size() ) * groups, WT_THREADS, 0, s, d_table, ch, row_stride, d_jump, int( W ), out_frames,
		d_blocks, num_blocks, plan.total_in, d_runs, d_index, d_win, groups, cpw, d_out );
	}

// the plan's per-block arrays for the *_synth_plan entry points: each nullable, filled up to `capacity`; returns the number of blocks
int64_t wt_plan_copy( const WtPlan & plan, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize,
	int32_t * ideal, int64_t * first_out, int32_t * num_out, int32_t * wanted, int64_t * in_start )
	{
	return wdl_export_plan( plan.blocks, int64_t( plan.blocks.size() ), capacity, offsets, fracpos, ratio, filtpos, oversize, ideal, first_out,
		[&]( int64_t i, const WtBlock & b ) { if( num_out ) num_out[i] = b.num_out; if( wanted ) wanted[i] = b.wanted; if( in_start ) in_start[i] = b.in_start; } );
	}

// Audio::synthesize_spectrum's loop: one row of W = 2^p frames shared by the channels, channel c reading it from jump_c on
constexpr int SP_MIN_POWER = 6, SP_MAX_POWER = 22;             // the tables flanhip_spectrum_table makes

int sp_synth_check( int64_t out_frames, double rate_out, int64_t ch, int32_t p, int64_t g, const float * freq, int64_t freq_count )
	{
	FLANHIP_REQUIRE( p >= SP_MIN_POWER && p <= SP_MAX_POWER, FLANHIP_ERR_UNSUPPORTED, "the table must hold 2^6 ... 2^22 frames" );
	FLANHIP_REQUIRE( ch > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( ch <= ( 1 << 16 ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	FLANHIP_REQUIRE( rate_out > 0.0 && std::isfinite( rate_out ), FLANHIP_ERR_INVALID_ARG, "output rate not positive" );
	return wt_synth_check( out_frames, 1.0f, int32_t( 1 ) << p, g, freq, freq_count );
	}

struct SpSynthLayout { WtSynthLayout wt; size_t jump_off, total; };
SpSynthLayout sp_synth_layout( int64_t ch, int64_t num_blocks, int64_t num_runs )
	{
	SpSynthLayout l;
	l.wt = wt_synth_layout( ch, num_blocks, num_runs );
	l.jump_off = ( l.wt.total + 15 ) & ~size_t( 15 );
	l.total = l.jump_off + sizeof( int32_t ) * size_t( ch );
	return l;
	}

int launch_sp_synth( const float * d_table, int32_t p, int64_t ch, int64_t out_frames, const WtPlan & plan, const std::vector<WtRun> & runs, float * d_out,
	void * d_ws, hipStream_t s )
	{
	const SpSynthLayout l = sp_synth_layout( ch, int64_t( plan.blocks.size() ), int64_t( runs.size() ) );
	std::vector<int32_t> jump( size_t( ch ), 0 );
	for( int64_t c = 0; c < ch; ++c ) jump[size_t( c )] = flanhip_spectrum_jump( c, ch, p );
	FLANHIP_CHECK( hipMemcpyAsync( ws_at<char>( d_ws, l.jump_off ), jump.data(), sizeof( int32_t ) * jump.size(), hipMemcpyHostToDevice, s ) );
	FLANHIP_CHECK( hipStreamSynchronize( s ) );
	const std::vector<float> index( size_t( ch ) * plan.blocks.size(), 0.0f );        // one slot: every block reads waveform 0
	return launch_wt_synth( d_table, ch, 0, ws_at<int32_t>( d_ws, l.jump_off ), int32_t( 1 ) << p, out_frames, plan, runs, index.data(), 0, d_out, d_ws, s );
	}

// ------------------------------------------------------------------------------------------------------------------------------------
// in-place edits

// grid: ch x slots.  Every slot is edited once (the reference's fade loops visit a slot once per channel, from racing threads).
__global__ __launch_bounds__( WT_THREADS ) void k_wt_edit( float * __restrict__ table, int W, int mode, int fade_frames )
	{
	__shared__ float s_red[WT_THREADS];
	const int lane = threadIdx.x;
	float * wf = table + int64_t( blockIdx.x ) * W;
	if( mode == FLANHIP_WAVETABLE_NORMALIZE || mode == FLANHIP_WAVETABLE_REMOVE_DC )
		{
		const bool is_max = mode == FLANHIP_WAVETABLE_NORMALIZE;
		float a = 0.0f;
		for( int f = lane; f < W; f += WT_THREADS ) a = is_max ? fmaxf( a, fabsf( wf[f] ) ) : a + wf[f];
		s_red[lane] = a;
		__syncthreads();
		for( int off = WT_THREADS / 2; off > 0; off >>= 1 )
			{
			if( lane < off ) s_red[lane] = is_max ? fmaxf( s_red[lane], s_red[lane + off] ) : s_red[lane] + s_red[lane + off];
			__syncthreads();
			}
		const float r = s_red[0];
		if( is_max )
			{
			if( double( r ) < 0.001 ) return;                                        // :447
			for( int f = lane; f < W; f += WT_THREADS ) wf[f] = wf[f] / r;
			}
		else
			{
			const float dc = r / float( W );                                         // :423
			for( int f = lane; f < W; f += WT_THREADS ) wf[f] = wf[f] - dc;
			}
		return;
		}
	// the fades (:375-380, :397-408): frame < fade_frames - 1 touches wf[frame] and wf[W - 1 - frame], in the order of the frames
	const bool jumps = mode == FLANHIP_WAVETABLE_REMOVE_JUMPS;
	const float mid = jumps ? ( wf[0] + wf[W - 1] ) / 2.0f : 0.0f;
	__syncthreads();                                                             // both ends are read before any frame is written
	const int F = fade_frames - 1 < W ? fade_frames - 1 : W;                     // (past the waveform the reference writes out of bounds)
	const float half_pi = 3.14159265358979323846f / 2.0f;
	for( int f = lane; f < W; f += WT_THREADS )
		{
		const int a = f, b = W - 1 - f;                                              // as a left frame, as a right frame
		if( a >= F && b >= F ) continue;
		float v = wf[f];
		const int first = a < b ? a : b, second = a < b ? b : a;
		const int frames[2] = { first, second };
		for( int u = 0; u < 2; ++u )
			{
			const int frame = frames[u];
			if( frame >= F ) continue;
			const float fade = sinf( half_pi * float( frame + 1 ) / float( fade_frames ) );
			v = jumps ? ( v - mid ) * fade + mid : v * fade;
			}
		wf[f] = v;
		}
	}

int wt_edit_check( const void * table, int64_t ch, int64_t slots, int32_t W, int mode, int32_t fade_frames )
	{
	FLANHIP_REQUIRE( table, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && slots > 0 && W > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( mode >= FLANHIP_WAVETABLE_NORMALIZE && mode <= FLANHIP_WAVETABLE_REMOVE_JUMPS, FLANHIP_ERR_INVALID_ARG, "unknown edit" );
	FLANHIP_REQUIRE( mode < FLANHIP_WAVETABLE_ADD_FADES || fade_frames >= 1, FLANHIP_ERR_INVALID_ARG, "fade_frames below 1" );
	FLANHIP_REQUIRE( ch * slots < ( int64_t( 1 ) << 31 ), FLANHIP_ERR_UNSUPPORTED, "too many waveforms" );
	return FLANHIP_OK;
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

int flanhip_wavetable_snap( const float * row, int64_t num_frames, int32_t frame_to_snap, float snap_height, int32_t search_distance, int32_t * out )
	{
	FLANHIP_REQUIRE( row && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && num_frames < ( int64_t( 1 ) << 31 ) && frame_to_snap >= 0 && frame_to_snap < num_frames, FLANHIP_ERR_INVALID_ARG,
		"the frame to snap lies outside the row" );
	*out = wt_snap( row, num_frames, frame_to_snap, snap_height, search_distance );
	return FLANHIP_OK;
	}

int flanhip_wavetable_starts( const float * row, int64_t num_frames, const float * local_wavelengths, int64_t num_locals, int32_t global_wavelength,
	int snap_mode, int pitch_mode, float snap_ratio, int32_t fixed_frame, volatile int * cancel, int32_t * out, int64_t capacity, int64_t * out_count )
	{
	FLANHIP_REQUIRE( row && out_count, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && num_frames < ( int64_t( 1 ) << 31 ), FLANHIP_ERR_INVALID_ARG, "row length out of range" );
	FLANHIP_REQUIRE( snap_mode >= FLANHIP_WAVETABLE_SNAP_NONE && snap_mode <= FLANHIP_WAVETABLE_SNAP_LEVEL, FLANHIP_ERR_INVALID_ARG, "unknown snap mode" );
	FLANHIP_REQUIRE( pitch_mode >= FLANHIP_WAVETABLE_PITCH_NONE && pitch_mode <= FLANHIP_WAVETABLE_PITCH_GLOBAL, FLANHIP_ERR_INVALID_ARG, "unknown pitch mode" );
	FLANHIP_REQUIRE( pitch_mode != FLANHIP_WAVETABLE_PITCH_LOCAL || local_wavelengths || num_locals == 0, FLANHIP_ERR_INVALID_ARG, "null local wavelengths" );
	FLANHIP_REQUIRE( num_locals >= 0 && capacity >= 0 && ( out || capacity == 0 ), FLANHIP_ERR_INVALID_ARG, "bad capacity" );
	FLANHIP_REQUIRE( fixed_frame >= 1, FLANHIP_ERR_INVALID_ARG, "fixed_frame below 1" );                       // :145
	FLANHIP_REQUIRE( snap_ratio > 0.0f && double( snap_ratio ) < .95, FLANHIP_ERR_INVALID_ARG, "snap_ratio outside ( 0, .95 )" );   // :146
	const int32_t ac_granularity = 128;                                          // :153
	auto snap_handler = [&]( int32_t frame_to_snap, int32_t snap_source_frame, int32_t max_snap )            // :167-179
		{
		if( snap_mode == FLANHIP_WAVETABLE_SNAP_ZERO ) return wt_snap( row, num_frames, frame_to_snap, 0.0f, max_snap );
		if( snap_mode == FLANHIP_WAVETABLE_SNAP_LEVEL ) return wt_snap( row, num_frames, frame_to_snap, row[snap_source_frame], max_snap );
		return frame_to_snap;
		};
	int64_t count = 0;
	int32_t back = snap_handler( 0, 0, wt_trunc( snap_ratio * float( global_wavelength ) ) );                   // :181
	if( count < capacity ) out[count] = back;
	++count;
	while( true )
		{
		if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
		int32_t expected_num_frames = 0;
		if( pitch_mode == FLANHIP_WAVETABLE_PITCH_LOCAL )
			{
			const int64_t local_wavelength_index = back / ac_granularity;            // :191 (an integer quotient under the floor)
			if( local_wavelength_index < 0 || local_wavelength_index >= num_locals ) break;
			const int32_t local_wavelength_c = wt_trunc( local_wavelengths[local_wavelength_index] );
			if( local_wavelength_c > 0 ) expected_num_frames = local_wavelength_c;
			else if( global_wavelength > 0 ) expected_num_frames = global_wavelength;
			else expected_num_frames = fixed_frame;
			}
		else if( pitch_mode == FLANHIP_WAVETABLE_PITCH_GLOBAL ) expected_num_frames = global_wavelength;
		else expected_num_frames = fixed_frame;
		if( int64_t( back ) + expected_num_frames >= num_frames ) break;         // :207
		// a length below 1 (a global wavelength of 0) keeps the reference's loop from ending; so does a snap that never moves forward
		FLANHIP_REQUIRE( expected_num_frames >= 1, FLANHIP_ERR_UNSUPPORTED, "an expected wavelength below one frame" );
		FLANHIP_REQUIRE( count <= 2 * num_frames, FLANHIP_ERR_UNSUPPORTED, "the walk does not advance" );
		const int32_t next = snap_handler( back + expected_num_frames, back, wt_trunc( snap_ratio * float( expected_num_frames ) ) );     // :210-213
		if( count < capacity ) out[count] = next;
		++count;
		back = next;
		}
	*out_count = count;
	return FLANHIP_OK;
	}

int flanhip_wavetable_table_index( const int32_t * starts, int64_t count, int32_t num_source_frames, const float * ratio, int64_t num, float * out )
	{
	FLANHIP_REQUIRE( starts && ratio && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count > 0 && num >= 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	for( int64_t i = 0; i < num; ++i )
		{
		const int32_t source_frame = wt_trunc( ratio[i] * float( num_source_frames ) );                      // :471
		float v;
		if( source_frame <= 0 ) v = 0.0f;
		else if( source_frame > num_source_frames ) v = float( count - 1 );
		else
			{
			const int32_t * right_iter = std::upper_bound( starts, starts + count, source_frame );
			const int64_t right_index = right_iter - starts;
			if( right_index == 0 ) v = 0.0f;
			else if( right_index == count ) v = float( count - 1 );
			else
				{
				const int32_t left_source_frame = *( right_iter - 1 ), right_source_frame = *right_iter;
				const float index = float( right_index - 1 ) + float( source_frame - left_source_frame ) / float( right_source_frame - left_source_frame );
				v = std::clamp( index, 0.0f, float( count - 1 ) );
				}
			}
		out[i] = v;
		}
	return FLANHIP_OK;
	}

int64_t flanhip_wavetable_slots( const int64_t * counts, int64_t num_channels )
	{
	if( !counts || num_channels <= 0 ) return 0;
	int64_t slots = 0;
	for( int64_t c = 0; c < num_channels; ++c ) slots = std::max( slots, counts[c] );
	return slots;
	}

size_t flanhip_wavetable_resample_workspace_bytes( int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts, int32_t wavelength )
	{
	static const float dummy = 0.0f;
	if( wt_resample_check( &dummy, num_channels, num_frames, starts, counts, wavelength, &dummy ) ) return 0;
	WtResamplePlan p;
	if( wt_resample_plan( num_channels, num_frames, starts, counts, &p ) ) return 0;
	return wt_resample_layout( p ).total;
	}

int flanhip_wavetable_resample_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts,
	int32_t wavelength, float * d_table, int32_t * d_rotations, void * d_workspace, void * stream )
	{
	if( int rc = wt_resample_check( d_audio, num_channels, num_frames, starts, counts, wavelength, d_table ) ) return rc;
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	WtResamplePlan p;
	if( int rc = wt_resample_plan( num_channels, num_frames, starts, counts, &p ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_wt_resample( d_audio, num_channels, num_frames, wavelength, p, d_table, d_rotations, d_workspace, (hipStream_t) stream );
	}

int flanhip_wavetable_resample( const float * audio, int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts,
	int32_t wavelength, float * table, int32_t * rotations, volatile int * cancel )
	{
	if( int rc = wt_resample_check( audio, num_channels, num_frames, starts, counts, wavelength, table ) ) return rc;
	WtResamplePlan p;
	if( int rc = wt_resample_plan( num_channels, num_frames, starts, counts, &p ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_x = nullptr; float * d_table = nullptr; int32_t * d_rot = nullptr; void * d_ws = nullptr;
	const size_t waves = size_t( num_channels ) * size_t( p.slots );
	if( int rc = call.in( audio, sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), &d_x ) ) return rc;
	if( int rc = call.out( table, sizeof( float ) * waves * size_t( wavelength ), &d_table ) ) return rc;
	if( int rc = call.out( rotations, sizeof( int32_t ) * waves, &d_rot ) ) return rc;      // (a null host pointer is not downloaded)
	if( int rc = call.scratch( wt_resample_layout( p ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_wt_resample( d_x, num_channels, num_frames, wavelength, p, d_table, d_rot, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int64_t flanhip_wavetable_synth_plan( int64_t out_frames, float sample_rate, int32_t wavelength, int64_t granularity_frames, const float * freq,
	int64_t freq_count, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize, int32_t * ideal,
	int64_t * first_out, int32_t * num_out, int32_t * wanted, int64_t * in_start )
	{
	if( int rc = wt_synth_check( out_frames, sample_rate, wavelength, granularity_frames, freq, freq_count ) ) return rc;
	WtPlan plan;
	if( int rc = wt_synth_plan( out_frames, wt_rate_out( sample_rate, wavelength ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	return wt_plan_copy( plan, capacity, offsets, fracpos, ratio, filtpos, oversize, ideal, first_out, num_out, wanted, in_start );
	}

int64_t flanhip_wavetable_synth_runs( int64_t out_frames, float sample_rate, int32_t wavelength, int64_t granularity_frames, const float * freq,
	int64_t freq_count, int64_t num_channels, int64_t capacity, int64_t * first_out, int32_t * num_out, int64_t * first_block, int32_t * num_blocks,
	int64_t * j0, int64_t * win_start, int32_t * win_len, int32_t * channels_per_group, int64_t * groups )
	{
	if( int rc = wt_synth_check( out_frames, sample_rate, wavelength, granularity_frames, freq, freq_count ) ) return rc;
	FLANHIP_REQUIRE( num_channels > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_channels <= ( 1 << 16 ), FLANHIP_ERR_UNSUPPORTED, "table out of range" );
	WtPlan plan;
	std::vector<WtRun> runs;
	if( int rc = wt_synth_plan( out_frames, wt_rate_out( sample_rate, wavelength ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	wt_runs( plan, &runs );
	int64_t grp = 0;
	const int cpw = wdl_channel_groups( out_frames, runs.size(), num_channels, &grp );
	if( channels_per_group ) *channels_per_group = cpw;
	if( groups ) *groups = grp;
	const int64_t fill = std::min<int64_t>( std::max<int64_t>( capacity, 0 ), int64_t( runs.size() ) );
	for( int64_t i = 0; i < fill; ++i )
		{
		const WtRun & r = runs[size_t( i )];
		if( first_out ) first_out[i] = r.first_out;
		if( num_out ) num_out[i] = r.num_out;
		if( first_block ) first_block[i] = r.first_block;
		if( num_blocks ) num_blocks[i] = r.num_blocks;
		if( j0 ) j0[i] = r.j0;
		if( win_start ) win_start[i] = r.win_start;
		if( win_len ) win_len[i] = r.win_len;
		}
	return int64_t( runs.size() );
	}

size_t flanhip_wavetable_synth_workspace_bytes( int64_t num_channels, int64_t out_frames, float sample_rate, int32_t wavelength, int64_t granularity_frames,
	const float * freq, int64_t freq_count )
	{
	if( num_channels <= 0 || wt_synth_check( out_frames, sample_rate, wavelength, granularity_frames, freq, freq_count ) ) return 0;
	WtPlan plan;
	std::vector<WtRun> runs;
	if( wt_synth_plan( out_frames, wt_rate_out( sample_rate, wavelength ), granularity_frames, freq, freq_count, &plan ) ) return 0;
	wt_runs( plan, &runs );
	return wt_synth_layout( num_channels, int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total;
	}

int flanhip_wavetable_synth_dev( const float * d_table, int64_t num_channels, int64_t slots, int32_t wavelength, float sample_rate, int64_t out_frames,
	int64_t granularity_frames, const float * freq, int64_t freq_count, const float * index, int64_t num_blocks, int smooth, float * d_out,
	void * d_workspace, void * stream )
	{
	if( int rc = wt_synth_check( out_frames, sample_rate, wavelength, granularity_frames, freq, freq_count ) ) return rc;
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	WtPlan plan;
	std::vector<WtRun> runs;
	if( int rc = wt_synth_plan( out_frames, wt_rate_out( sample_rate, wavelength ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	if( int rc = wt_synth_args( d_table, num_channels, slots, wavelength, index, num_blocks, plan, d_out ) ) return rc;
	wt_runs( plan, &runs );
	if( int rc = require_device() ) return rc;
	return launch_wt_synth( d_table, num_channels, slots * wavelength, nullptr, wavelength, out_frames, plan, runs, index, smooth, d_out, d_workspace, (hipStream_t) stream );
	}

int flanhip_wavetable_synth( const float * table, int64_t num_channels, int64_t slots, int32_t wavelength, float sample_rate, int64_t out_frames,
	int64_t granularity_frames, const float * freq, int64_t freq_count, const float * index, int64_t num_blocks, int smooth, float * out,
	volatile int * cancel )
	{
	if( int rc = wt_synth_check( out_frames, sample_rate, wavelength, granularity_frames, freq, freq_count ) ) return rc;
	WtPlan plan;
	std::vector<WtRun> runs;
	if( int rc = wt_synth_plan( out_frames, wt_rate_out( sample_rate, wavelength ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	if( int rc = wt_synth_args( table, num_channels, slots, wavelength, index, num_blocks, plan, out ) ) return rc;
	wt_runs( plan, &runs );
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_table = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( table, sizeof( float ) * size_t( num_channels ) * size_t( slots ) * size_t( wavelength ), &d_table ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( out_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( wt_synth_layout( num_channels, int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_wt_synth( d_table, num_channels, slots * wavelength, nullptr, wavelength, out_frames, plan, runs, index, smooth, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

// ---- the loop of Audio::synthesize_spectrum (AudioSynthesis.cpp:230-263): the same resampler over ONE table row of W = 2^p frames, which
// every channel reads at its own phase offset; one slot, no blend

int64_t flanhip_spectrum_synth_plan( int64_t out_frames, double rate_out, int64_t granularity_frames, const float * freq, int64_t freq_count,
	int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize, int32_t * ideal, int64_t * first_out,
	int32_t * num_out, int32_t * wanted, int64_t * in_start )
	{
	if( int rc = sp_synth_check( out_frames, rate_out, 1, 6, granularity_frames, freq, freq_count ) ) return rc;
	WtPlan plan;
	if( int rc = wt_synth_plan( out_frames, std::max( rate_out, 1.0 ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	return wt_plan_copy( plan, capacity, offsets, fracpos, ratio, filtpos, oversize, ideal, first_out, num_out, wanted, in_start );
	}

size_t flanhip_spectrum_synth_workspace_bytes( int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames, int64_t granularity_frames,
	const float * freq, int64_t freq_count )
	{
	if( sp_synth_check( out_frames, rate_out, num_channels, table_size_power, granularity_frames, freq, freq_count ) ) return 0;
	WtPlan plan;
	std::vector<WtRun> runs;
	if( wt_synth_plan( out_frames, std::max( rate_out, 1.0 ), granularity_frames, freq, freq_count, &plan ) ) return 0;
	wt_runs( plan, &runs );
	return sp_synth_layout( num_channels, int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total;
	}

int flanhip_spectrum_synth_dev( const float * d_table, int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames,
	int64_t granularity_frames, const float * freq, int64_t freq_count, float * d_out, void * d_workspace, void * stream )
	{
	if( int rc = sp_synth_check( out_frames, rate_out, num_channels, table_size_power, granularity_frames, freq, freq_count ) ) return rc;
	FLANHIP_REQUIRE( d_table && d_out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	WtPlan plan;
	std::vector<WtRun> runs;
	if( int rc = wt_synth_plan( out_frames, std::max( rate_out, 1.0 ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	wt_runs( plan, &runs );
	if( int rc = require_device() ) return rc;
	return launch_sp_synth( d_table, table_size_power, num_channels, out_frames, plan, runs, d_out, d_workspace, (hipStream_t) stream );
	}

int flanhip_spectrum_synth( const float * table, int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames,
	int64_t granularity_frames, const float * freq, int64_t freq_count, float * out, volatile int * cancel )
	{
	if( int rc = sp_synth_check( out_frames, rate_out, num_channels, table_size_power, granularity_frames, freq, freq_count ) ) return rc;
	FLANHIP_REQUIRE( table && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	WtPlan plan;
	std::vector<WtRun> runs;
	if( int rc = wt_synth_plan( out_frames, std::max( rate_out, 1.0 ), granularity_frames, freq, freq_count, &plan ) ) return rc;
	wt_runs( plan, &runs );
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_table = nullptr; float * d_out = nullptr; void * d_ws = nullptr;
	if( int rc = call.in( table, sizeof( float ) << table_size_power, &d_table ) ) return rc;
	if( int rc = call.out( out, sizeof( float ) * size_t( num_channels ) * size_t( out_frames ), &d_out ) ) return rc;
	if( int rc = call.scratch( sp_synth_layout( num_channels, int64_t( plan.blocks.size() ), int64_t( runs.size() ) ).total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_sp_synth( d_table, table_size_power, num_channels, out_frames, plan, runs, d_out, d_ws, nullptr ) ) return rc;
	return call.finish();
	}

int flanhip_wavetable_edit_dev( float * d_table, int64_t num_channels, int64_t slots, int32_t wavelength, int mode, int32_t fade_frames, void * stream )
	{
	if( int rc = wt_edit_check( d_table, num_channels, slots, wavelength, mode, fade_frames ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_kernel( __func__, k_wt_edit, num_channels * slots, WT_THREADS, 0, (hipStream_t) stream, d_table, int( wavelength ), mode, int( fade_frames ) );
	}

int flanhip_wavetable_edit( float * table, int64_t num_channels, int64_t slots, int32_t wavelength, int mode, int32_t fade_frames, volatile int * cancel )
	{
	if( int rc = wt_edit_check( table, num_channels, slots, wavelength, mode, fade_frames ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	float * d_table = nullptr;
	const size_t bytes = sizeof( float ) * size_t( num_channels ) * size_t( slots ) * size_t( wavelength );
	if( int rc = call.out( table, bytes, &d_table ) ) return rc;
	if( int rc = flanhip_upload( d_table, table, bytes ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_kernel( __func__, k_wt_edit, num_channels * slots, WT_THREADS, 0, nullptr, d_table, int( wavelength ), mode, int( fade_frames ) ) ) return rc;
	return call.finish();
	}

} // extern "C"
