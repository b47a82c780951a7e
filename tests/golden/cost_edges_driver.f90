!  cost_edges_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference modules, compiled by tests/golden/make_cost_edges.py against the module files and
!  objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).  One entry:
!    ce_run   mwd_cost::compute_jobs, MWD_COST_DIFF::COMPUTE_JOBS_B (twice: jobs_b = rcfg(3) and rcfg(4)) and COMPUTE_JOBS_D on a
!             PRESCRIBED discharge (smash/solver/optimize/mwd_cost.f90:37-156, smash/solver/forward/forward_db.f90:2445-2715)
!  It fills the least of setup, mesh, input_data and output that those routines read.
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module cost_edges_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mwd_output
    use mwd_cost, only: compute_jobs
    use mwd_cost_diff, only: compute_jobs_b, compute_jobs_d
    use mwd_output_diff, only: OutputDiffSide => OUTPUTDT, OUTPUTDT_DIFF

    implicit none

contains

    function crit_name(code) result(s)
        integer, intent(in) :: code
        character(20) :: s
        select case (code)
        case (1); s = "nse"
        case (2); s = "kge"
        case (3); s = "kge2"
        case (4); s = "se"
        case (5); s = "rmse"
        case (6); s = "logarithmic"
        case default; s = "..."
        end select
    end function crit_name

    !  icfg = (nrow; ncol; nt; ng; optimize_start_step; njf)      rcfg = (dt; dx; first jobs_b; second jobs_b)
    !  arrays column-major as the reference holds them, gauge_pos 1-based
    !  res = (jobs of compute_jobs; jobs_d of COMPUTE_JOBS_D; jobs of COMPUTE_JOBS_D: assigned only where there is a median, and from the
    !  tangent criteria's own primal expressions, which differ from compute_jobs' in the last bit; not recorded)
    subroutine ce_run(icfg, rcfg, flwacc, gauge_pos, area, qobs, qsim, qsim_d, wgauge, jobs_codes, wjobs, &
    & res, qsim_b1, qsim_b2) bind(C, name="ce_run")

        integer(c_int), intent(in) :: icfg(6)
        real(c_float), intent(in) :: rcfg(4)
        integer(c_int), intent(in) :: flwacc(icfg(1), icfg(2))
        integer(c_int), intent(in) :: gauge_pos(icfg(4), 2)
        real(c_float), intent(in) :: area(icfg(4))
        real(c_float), intent(in) :: qobs(icfg(4), icfg(3)), qsim(icfg(4), icfg(3)), qsim_d(icfg(4), icfg(3))
        real(c_float), intent(in) :: wgauge(icfg(4))
        integer(c_int), intent(in) :: jobs_codes(icfg(6))
        real(c_float), intent(in) :: wjobs(icfg(6))
        real(c_float), intent(inout) :: res(3), qsim_b1(icfg(4), icfg(3)), qsim_b2(icfg(4), icfg(3))

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        type(OutputDT) :: output
        type(OutputDiffSide) :: out_side
        type(OUTPUTDT_DIFF) :: out_side_b, out_side_d
        real(sp) :: jobs, jobs_b, jobs_d
        integer :: nrow, ncol, nt, ng, njf, j

        nrow = icfg(1); ncol = icfg(2); nt = icfg(3); ng = icfg(4); njf = icfg(6)
        setup%structure = "gr-a"
        setup%dt = rcfg(1)
        setup%ntime_step = nt
        setup%mean_forcing = .true.
        call SetupDT_initialise(setup, 0, ng)

        call MeshDT_initialise(mesh, setup, nrow, ncol, ng)
        mesh%dx = rcfg(2)
        mesh%flwacc = flwacc
        mesh%active_cell = 1
        mesh%nac = nrow*ncol
        mesh%gauge_pos = gauge_pos
        mesh%area = area

        call Input_DataDT_initialise(input_data, setup, mesh)
        input_data%qobs = qobs
        input_data%mean_prcp = 0._sp

        call OutputDT_initialise(output, setup, mesh)
        output%qsim = qsim

        setup%optimize%optimize_start_step = icfg(5)
        setup%optimize%njf = njf
        deallocate (setup%optimize%jobs_fun, setup%optimize%wjobs_fun)
        allocate (setup%optimize%jobs_fun(njf), setup%optimize%wjobs_fun(njf))
        do j = 1, njf
            setup%optimize%jobs_fun(j) = crit_name(jobs_codes(j))
            setup%optimize%wjobs_fun(j) = wjobs(j)
        end do
        setup%optimize%wgauge = wgauge
        setup%optimize%mask_event = 0

        jobs = 0._sp
        call compute_jobs(setup, mesh, input_data, output, jobs)
        res(1) = jobs

        allocate (out_side%qsim(ng, nt), out_side_b%qsim(ng, nt), out_side_d%qsim(ng, nt))
        out_side%qsim = qsim
        out_side_b%qsim = 0._sp
        jobs = 0._sp
        jobs_b = rcfg(3)
        call compute_jobs_b(setup, mesh, input_data, out_side, out_side_b, jobs, jobs_b)
        qsim_b1 = out_side_b%qsim

        out_side%qsim = qsim
        out_side_b%qsim = 0._sp
        jobs = 0._sp
        jobs_b = rcfg(4)
        call compute_jobs_b(setup, mesh, input_data, out_side, out_side_b, jobs, jobs_b)
        qsim_b2 = out_side_b%qsim

        out_side%qsim = qsim
        out_side_d%qsim = qsim_d
        jobs = 0._sp
        jobs_d = 0._sp
        call compute_jobs_d(setup, mesh, input_data, out_side, out_side_d, jobs, jobs_d)
        res(2) = jobs_d
        res(3) = jobs

    end subroutine ce_run

end module cost_edges_driver
